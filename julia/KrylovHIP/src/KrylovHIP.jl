# KrylovHIP.jl -- Krylov.jl on libkrylov_hip.so (hand-written gfx950 kernels behind a C ABI, include/krylov_hip.h).
#
# Two layers, both through `ccall`:
#
#   1. The extension contract of Krylov.jl (docs/src/custom_workspaces.md:107-300): a device vector type `HIPVector`, a device
#      matrix type `HIPMatrix` (block solvers) and a CSR operator `HIPCsr` with methods for every `Krylov.k*` primitive and
#      `kmul!`.  With these the UNMODIFIED solvers of Krylov.jl run on the GPU, one kernel launch per primitive
#      (all 35+ solvers; 249 it/s for cg! at 512^3).
#
#   2. Method specialisations of `cg!`, `gmres!`, `bicgstab!` and `block_gmres!` for workspaces whose storage type is
#      `HIPVector` / `HIPMatrix` and an operator that is a `HIPCsr`.  They hand the device pointers of the WORKSPACE'S OWN
#      vectors to the library (`khip_*_workspace_adopt`, include/krylov_hip.h) and run its fused, device-resident loop on them
#      (`khip_*_solve`; 310-316 it/s for cg! at 512^3): `solution(ws) === ws.x`, `ws.stats` is filled as the generic method fills
#      it, nothing is copied.
#
#      EVERY entry point of the reference reaches them.  `cg(A, b)`, `krylov_solve(Val(:cg), A, b)`, `krylov_solve!(ws, A, b)`
#      and the `x0` forms are generated methods that forward ALL keywords to `cg!(ws, A, b; ...)` explicitly -- including their
#      own default `callback = workspace -> false` (src/cg.jl:110; src/interface.jl:146-154, 160-170, 306-320).  `user_callback`
#      below recognises those defaults (anonymous functions of module Krylov that capture nothing) as "no callback", so the
#      device-resident loop is what `x, stats = cg(A_gpu, b_gpu)` runs; `NATIVE_SOLVES[]` / `LAST_PATH[]` record it and
#      test/runtests.jl asserts on them.  A REAL callback runs inside the library's host-driven loop on the fused kernels through a
#      `@cfunction` trampoline (`khip_options.callback`): it sees the workspace's own vectors and the residual history so far.
#      What the library cannot take (`ldiv = true`, a preconditioner that is not a `HIPOperator`, a verbose log into a non-file
#      `IO`) falls back to the generic method of layer 1 with `invoke` on the fully parametrised generic signature: same
#      results, primitive by primitive.
#
# Julia is not installed in the image this library is built in: this file is checked mechanically (tests/test_abi.py parses every
# `ccall` against include/krylov_hip.h -- symbol, arity, return and argument types -- and checks that every `k*` primitive the
# reference solvers call has a method here), and the same entry points, in the same order, are executed by the Python mirror
# (krylov.jl_amd/__init__.py, whose workspaces adopt their own vectors exactly as below) and by tests/c/adopt_sequence.c.
module KrylovHIP

using Krylov, LinearAlgebra, SparseArrays
import Krylov: kdot, kdotr, knorm, kscal!, kdiv!, kcopy!, kscalcopy!, kdivcopy!, kaxpy!, kaxpby!, kfill!, kref!, kmul!
import Krylov: CgWorkspace, GmresWorkspace, BicgstabWorkspace, BlockGmresWorkspace

export Ctx, CTX, HIPVector, HIPMatrix, HIPCsr, HIPOperator, jacobi, ilu0

# krylov.jl_amd/libkrylov_hip.so of this repository, or wherever KHIP_LIBRARY points
const lib = get(ENV, "KHIP_LIBRARY", normpath(joinpath(@__DIR__, "..", "..", "..", "krylov.jl_amd", "libkrylov_hip.so")))

ck(rc) = rc == 0 || error(unsafe_string(ccall((:khip_last_error, lib), Cstring, ())))

# ------------------------------------------------------------------------------------------------ context
mutable struct Ctx; h::Ptr{Cvoid}; end
function Ctx(device::Integer = 0)
  major = Ref{Cint}(); minor = Ref{Cint}()
  ccall((:khip_version, lib), Cvoid, (Ref{Cint}, Ref{Cint}), major, minor)
  (major[] == 0 && minor[] >= 4) || error("libkrylov_hip $(major[]).$(minor[]) lacks khip_*_last_path / the adopt entry points (need >= 0.4)")
  r = Ref{Ptr{Cvoid}}(); ck(ccall((:khip_ctx_create, lib), Cint, (Cint, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), device, C_NULL, r))
  Ctx(r[])
end
const CTX = Ref{Ctx}()                            # one context per process (one process per GPU)
synchronize() = ck(ccall((:khip_ctx_sync, lib), Cint, (Ptr{Cvoid},), CTX[].h))

# ------------------------------------------------------------------------------------------------ device vector: the storage type S
mutable struct HIPVector <: AbstractVector{Float64}
  ptr::Ptr{Float64}; n::Int
  function HIPVector(::UndefInitializer, n::Integer)          # S(undef, n) / S(undef, 0) -- src/krylov_workspaces.jl:269-285
    r = Ref{Ptr{Cvoid}}(C_NULL)
    n > 0 && ck(ccall((:khip_malloc, lib), Cint, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), CTX[].h, 8n, r))
    v = new(Ptr{Float64}(r[]), n)
    finalizer(x -> ccall((:khip_free, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), CTX[].h, x.ptr), v)
  end
end
Base.size(v::HIPVector) = (v.n,);  Base.length(v::HIPVector) = v.n
Base.similar(v::HIPVector) = HIPVector(undef, v.n)
Base.similar(v::HIPVector, ::Type{Float64}, dims::Dims{1}) = HIPVector(undef, dims[1])
Base.getindex(::HIPVector, i...) = error("scalar indexing of a device vector")   # like allowscalar(false), test/gpu/amd.jl:8
Krylov.ktypeof(::HIPVector) = HIPVector                                          # src/krylov_utils.jl:204-224
function HIPVector(x::AbstractVector{<:Real}); xh = Vector{Float64}(x); v = HIPVector(undef, length(xh))
  ck(ccall((:khip_memcpy_h2d, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), CTX[].h, v.ptr, xh, 8length(xh))); v; end
function Base.Vector(v::HIPVector); x = Vector{Float64}(undef, v.n)
  ck(ccall((:khip_memcpy_d2h, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), CTX[].h, x, v.ptr, 8v.n)); x; end
Base.Array(v::HIPVector) = Vector(v)
Base.copy(v::HIPVector) = kcopy!(v.n, similar(v), v)
Base.show(io::IO, v::HIPVector) = print(io, "HIPVector(", v.n, ")")
Base.show(io::IO, ::MIME"text/plain", v::HIPVector) = show(io, v)

# ------------------------------------------------------------------------------------------------ k* primitives: one ccall each
# (src/krylov_utils.jl line in the comment)
function kdot(n::Integer, x::HIPVector, y::HIPVector)                                       # :309-311
  r = Ref{Cdouble}(); ck(ccall((:khip_dot, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}), CTX[].h, n, x.ptr, y.ptr, r)); r[]
end
kdotr(n::Integer, x::HIPVector, y::HIPVector) = kdot(n, x, y)                                 # :313-314
function knorm(n::Integer, x::HIPVector)                                                     # :316-317
  r = Ref{Cdouble}(); ck(ccall((:khip_nrm2, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ref{Cdouble}), CTX[].h, n, x.ptr, r)); r[]
end
kscal!(n::Integer, s::Float64, x::HIPVector) = (ck(ccall((:khip_scal, lib), Cint, (Ptr{Cvoid}, Int64, Cdouble, Ptr{Cdouble}), CTX[].h, n, s, x.ptr)); x)                      # :321-323
kdiv!(n::Integer, x::HIPVector, s::Float64) = (ck(ccall((:khip_div, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Cdouble), CTX[].h, n, x.ptr, s)); x)                        # :325-326
kcopy!(n::Integer, y::HIPVector, x::HIPVector) = (ck(ccall((:khip_copy, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}), CTX[].h, n, y.ptr, x.ptr)); y)           # :328-329 (dest, src)
kscalcopy!(n::Integer, y::HIPVector, s::Float64, x::HIPVector) = (ck(ccall((:khip_scalcopy, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}), CTX[].h, n, y.ptr, s, x.ptr)); y)   # :331-332
kdivcopy!(n::Integer, y::HIPVector, x::HIPVector, s::Float64) = (ck(ccall((:khip_divcopy, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble), CTX[].h, n, y.ptr, x.ptr, s)); y)     # :334-335
kaxpy!(n::Integer, s::Float64, x::HIPVector, y::HIPVector) = (ck(ccall((:khip_axpy, lib), Cint, (Ptr{Cvoid}, Int64, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}), CTX[].h, n, s, x.ptr, y.ptr)); y)            # :337-339
kaxpby!(n::Integer, s::Float64, x::HIPVector, t::Float64, y::HIPVector) = (ck(ccall((:khip_axpby, lib), Cint, (Ptr{Cvoid}, Int64, Cdouble, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}), CTX[].h, n, s, x.ptr, t, y.ptr)); y)  # :341-345
kfill!(x::HIPVector, val::Float64) = (ck(ccall((:khip_fill, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Cdouble), CTX[].h, x.n, x.ptr, val)); x)                           # :347
kref!(n::Integer, x::HIPVector, y::HIPVector, c::Float64, s::Float64) = (ck(ccall((:khip_ref, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble), CTX[].h, n, x.ptr, y.ptr, c, s)); (x, y))  # :349

# ------------------------------------------------------------------------------------------------ operator: size, eltype, kmul!
# (docs/src/matrix_free.md:32-34)
mutable struct HIPCsr; h::Ptr{Cvoid}; m::Int; n::Int; adj::Union{Nothing,HIPCsr}; end      # adj: A' once it has been built
HIPCsr(h::Ptr{Cvoid}, m::Integer, n::Integer) = HIPCsr(h, m, n, nothing)
destroy_csr(A::HIPCsr) = ccall((:khip_csr_destroy, lib), Cint, (Ptr{Cvoid},), A.h)
function HIPCsr(A::SparseArrays.SparseMatrixCSC{Float64,<:Integer})    # CSC of a symmetric matrix == its CSR;
  At = SparseArrays.sparse(A')                                         # general case: CSR of A = CSC of A'
  r = Ref{Ptr{Cvoid}}()
  ck(ccall((:khip_csr_create, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{Int32}, Ptr{Cdouble}, Cint, Cint, Ref{Ptr{Cvoid}}),
           CTX[].h, size(A, 1), size(A, 2), SparseArrays.nnz(At), Int64.(At.colptr), 64, Int32.(At.rowval), At.nzval, 1, 0, r))   # index_base = 1
  finalizer(destroy_csr, HIPCsr(r[], size(A)...))
end
Base.size(A::HIPCsr) = (A.m, A.n);  Base.size(A::HIPCsr, i::Integer) = i == 1 ? A.m : (i == 2 ? A.n : 1);  Base.eltype(::HIPCsr) = Float64
kmul!(y::HIPVector, A::HIPCsr, x::HIPVector) = (ck(ccall((:khip_spmv, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), CTX[].h, A.h, x.ptr, y.ptr)); y)   # src/krylov_utils.jl:305
kmul!(y::HIPVector, ::UniformScaling, x::HIPVector) = kcopy!(length(x), y, x)   # the unguarded mul!(v, I, q) of src/bicgstab.jl:222
LinearAlgebra.mul!(y::HIPVector, A::HIPCsr, x::HIPVector) = kmul!(y, A, x)
Base.:*(A::HIPCsr, x::HIPVector) = kmul!(HIPVector(undef, A.m), A, x)
# adjoint products for the solvers that need A' (LSQR, LSMR, BiLQ, QMR, ...; they write `Aᴴ = A'` once per solve): the transposed
# operator is built ONCE per matrix (khip_csr_transpose makes an independent handle), cached in `A.adj`, owned by a finalizer of its
# own, and points back so that (A')' === A.  Repeated solves neither rebuild nor leak it.
function Base.adjoint(A::HIPCsr)
  A.adj === nothing || return A.adj
  r = Ref{Ptr{Cvoid}}()
  ck(ccall((:khip_csr_transpose, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), CTX[].h, A.h, r))
  At = finalizer(destroy_csr, HIPCsr(r[], A.n, A.m, A))
  A.adj = At
  return At
end
Base.transpose(A::HIPCsr) = adjoint(A)            # real element type

# ------------------------------------------------------------------------------------------------ C structs of the solver entries
struct Operator                     # khip_operator, include/krylov_hip.h
  csr::Ptr{Cvoid}; apply::Ptr{Cvoid}; self::Ptr{Cvoid}
end
Operator(A::HIPCsr) = Operator(A.h, C_NULL, C_NULL)

struct Options                      # khip_options: same members, same order (isbits struct = the C layout)
  atol::Cdouble; rtol::Cdouble; itmax::Cint; timemax::Cdouble; history::Cint; radius::Cdouble; linesearch::Cint
  restart::Cint; reorthogonalization::Cint; fused::Cint; callback::Ptr{Cvoid}; callback_data::Ptr{Cvoid}
  variant::Cint; verbose::Cint; log_fd::Cint
end
function Options(; atol, rtol, itmax, timemax, history, radius = 0.0, linesearch = false, restart = false, reorthogonalization = false,
                 fused = 2, variant = 0, verbose = 0, log_fd = 0, callback = C_NULL, callback_data = C_NULL)
  # timemax: NaN or <= 0 means "no limit" on the C side (include/krylov_hip.h); itmax above the Cint range is "no limit" too.
  # A time limit the entry point has already used up (`timemax -= elapsed_time`, src/interface.jl:151) must stay a limit: the
  # smallest positive one.
  tm = isfinite(timemax) ? max(timemax, floatmin(Float64)) : NaN
  Options(atol, rtol, Cint(clamp(itmax, 0, typemax(Cint))), tm, history, radius, linesearch, restart,
          reorthogonalization, fused, callback, callback_data, variant, verbose, log_fd)
end

struct Stats                        # khip_stats
  niter::Cint; solved::Cint; inconsistent::Cint; indefinite::Cint; npcCount::Cint
  timer::Cdouble; status::NTuple{96,UInt8}; residuals::Ptr{Cdouble}; nres::Cint; error::NTuple{160,UInt8}; allocation_timer::Cdouble
end
cstr(t::NTuple{N,UInt8}) where N = (b = collect(t); i = findfirst(==(0x00), b); String(b[1:(i === nothing ? N : i - 1)]))

# native operators for the M / N arguments (z <- M r on device pointers): Jacobi and ILU(0) / IC(0)
mutable struct HIPOperator
  op::Base.RefValue{Operator}; n::Int; kind::Symbol; A::HIPCsr          # A must outlive the operator
end
function jacobi(A::HIPCsr); op = Ref(Operator(C_NULL, C_NULL, C_NULL))
  ck(ccall((:khip_jacobi_create, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Operator}), CTX[].h, A.h, op))
  finalizer(x -> ccall((:khip_jacobi_destroy, lib), Cint, (Ref{Operator},), x.op), HIPOperator(op, A.m, :jacobi, A)); end
function ilu0(A::HIPCsr); op = Ref(Operator(C_NULL, C_NULL, C_NULL))      # IC(0) for SPD A: docs/src/gpu.md:74-163 without the vendor library
  ck(ccall((:khip_ilu0_create, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Operator}), CTX[].h, A.h, op))
  finalizer(x -> ccall((:khip_ilu0_destroy, lib), Cint, (Ref{Operator},), x.op), HIPOperator(op, A.m, :ilu0, A)); end
Base.size(M::HIPOperator) = (M.n, M.n);  Base.eltype(::HIPOperator) = Float64
# the generic solvers apply M through mulorldiv! -> mul!(y, M, x) (src/krylov_utils.jl:307): call the operator's own `apply`
function LinearAlgebra.mul!(y::HIPVector, M::HIPOperator, x::HIPVector)
  rc = ccall(M.op[].apply, Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), M.op[].self, x.ptr, y.ptr)
  rc == 0 || error("preconditioner application failed"); y
end
kmul!(y::HIPVector, M::HIPOperator, x::HIPVector) = mul!(y, M, x)

# ------------------------------------------------------------------------------------------------ shared pieces of the forwarding methods
# Julia workspace -> its khip_*_workspace handle: adopted once, destroyed by the workspace's finalizer.  Weak keys (identity of the mutable
# workspace): the table must not keep a workspace alive.  The finalizers capture the handle and do not touch the table.
const HANDLES = WeakKeyDict{Any,Ptr{Cvoid}}()
dptr(v::HIPVector) = isempty(v) ? Ptr{Cdouble}(C_NULL) : v.ptr
native_precond(M) = M === I || M isa HIPOperator
opref(M) = M === I ? Ptr{Operator}(C_NULL) : Base.unsafe_convert(Ptr{Operator}, M.op)
# verbose log: the C loop writes with dprintf to a file descriptor (options.log_fd, 0 = stdout)
# (`fd(::IOStream)` is an `Int` in older and a `RawFD` in newer Julia versions: `cconvert` takes both)
logfd(io::IO) = (io === Krylov.kstdout || io === stdout) ? Cint(0) : (io isa IOStream ? Base.cconvert(Cint, fd(io))::Cint : Cint(-1))
native_log(verbose, io) = verbose <= 0 || logfd(io) >= 0

# ---- callbacks ------------------------------------------------------------------------------------------------------------
# The reference's generated entry points pass `callback = workspace -> false` EXPLICITLY (see the header of this file): one
# anonymous function per generated method, all defined in module Krylov, none capturing anything.  Those are "no callback".
default_callback(cb) = parentmodule(typeof(cb)) === Krylov && Base.issingletontype(typeof(cb))
user_callback(cb) = (cb === nothing || default_callback(cb)) ? nothing : cb
# A user's callback runs inside the library's host-driven loop (khip_options.callback, include/krylov_hip.h): the trampoline
# brings the residual history of the C side into `ws.stats.residuals` (what the reference's callbacks read, docs/src/callbacks.md),
# calls `callback(ws)::Bool` and keeps an exception for after the solve (nothing may unwind through the C frames).
mutable struct CallbackBox
  f::Any; ws::Any; stats::Ptr{Cvoid}; history::Bool; err::Any
end
function callback_trampoline(_::Ptr{Cvoid}, ud::Ptr{Cvoid})::Cint
  box = unsafe_pointer_to_objref(ud)::CallbackBox
  try
    if box.history
      st = unsafe_load(Ptr{Stats}(box.stats)); res = box.ws.stats.residuals
      for i in (length(res) + 1):Int(st.nres); push!(res, unsafe_load(st.residuals, i)); end
    end
    return box.f(box.ws) ? Cint(1) : Cint(0)
  catch e
    box.err = e
    return Cint(1)                                 # stop the solve; `finish_callback` rethrows
  end
end
const CALLBACK = Ref{Ptr{Cvoid}}(C_NULL)
# (callback, callback_data) of khip_options and the box to GC.@preserve; `stats_ptr` = khip_*_stats(h) (stable per handle)
function callback_args(cb, ws, stats_ptr::Ptr{Stats}, history::Bool)
  cb === nothing && return C_NULL, C_NULL, nothing
  history && empty!(ws.stats.residuals)
  box = CallbackBox(cb, ws, Ptr{Cvoid}(stats_ptr), history, nothing)
  return CALLBACK[], pointer_from_objref(box), box
end
finish_callback(box) = (box !== nothing && box.err !== nothing) ? throw(box.err) : nothing

# how many solves took the library's loop, and which loop the last one ran (khip_*_last_path: 2 = device-resident / look-ahead,
# 1 = host-driven on the fused kernels, 0 = one launch per primitive) -- test/runtests.jl asserts on both after every entry point
const NATIVE_SOLVES = Ref(0)
const LAST_PATH = Ref(-1)
const GENERIC_SOLVES = Ref(0)                      # solves handed to the generic method by `invoke`

function fill_stats!(stats::Krylov.SimpleStats{Float64}, sp::Ptr{Stats}, history::Bool)
  st = unsafe_load(sp)
  Krylov.reset!(stats)
  history && st.nres > 0 && append!(stats.residuals, unsafe_wrap(Array, st.residuals, Int(st.nres)))
  stats.niter = st.niter;  stats.solved = st.solved != 0;  stats.inconsistent = st.inconsistent != 0
  stats.indefinite = st.indefinite != 0;  stats.npcCount = st.npcCount
  stats.timer = st.timer;  stats.status = cstr(st.status)
  return st
end
# a failed solve throws what the generic method throws: error(...) with the library's message (argument errors, SPD violation)
failed(st::Stats) = error(isempty(cstr(st.error)) ? unsafe_string(ccall((:khip_last_error, lib), Cstring, ())) : cstr(st.error))

# ------------------------------------------------------------------------------------------------ cg!  (src/cg.jl:120-291)
const CgWs = CgWorkspace{Float64,Float64,HIPVector}
function cg_handle(ws::CgWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_cg_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.x.ptr, ws.r.ptr, ws.p.ptr, ws.Ap.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_cg_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
cg_adopt(h, name, v::HIPVector) = ck(ccall((:khip_cg_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

function Krylov.cg!(ws::CgWs, A::HIPCsr, b::HIPVector; M = I, ldiv::Bool = false, radius::Float64 = 0.0, linesearch::Bool = false,
                    atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0, timemax::Float64 = Inf,
                    verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  if ldiv || !native_precond(M) || !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.cg!, Tuple{CgWs,Any,AbstractVector{Float64}}, ws, A, b; M, ldiv, radius, linesearch, atol, rtol, itmax, timemax, verbose,
                  history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # the reference's own argument checks, :128-139
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  m == n || error("System must be square")
  length(b) == n || error("Inconsistent problem size")
  linesearch && (radius > 0) && error("`linesearch` set to `true` but trust-region radius > 0")
  (ws.warm_start && linesearch) && error("warm_start and linesearch cannot be used together")
  Krylov.allocate_if(M !== I, ws, :z, HIPVector, ws.x)                                       # :142
  Krylov.allocate_if(linesearch || (radius > 0), ws, :npc_dir, HIPVector, ws.x)              # :143
  h = cg_handle(ws)
  for (name, v) in (("x", ws.x), ("r", ws.r), ("p", ws.p), ("Ap", ws.Ap), ("z", ws.z), ("npc_dir", ws.npc_dir), ("dx", ws.Δx))
    cg_adopt(h, name, v)                                                                    # the fields as they are NOW (pointer hand-over only)
  end
  ws.warm_start && ck(ccall((:khip_cg_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, ws.Δx.ptr))   # Δx already holds x0: sets the flag
  sp = ccall((:khip_cg_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, radius, linesearch, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  opA = Ref(Operator(A))
  rc = GC.@preserve ws A b M opts opA box ccall((:khip_cg_solve, lib), Cint, (Ptr{Cvoid}, Ref{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ref{Options}),
                                                 h, opA, opref(M), b.ptr, opts)
  st = fill_stats!(ws.stats, sp, history)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_cg_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ gmres!  (src/gmres.jl:121-384)
const GmresWs = GmresWorkspace{Float64,Float64,HIPVector}
basis_ptrs(V::Vector{HIPVector}) = Ptr{Cdouble}[v.ptr for v in V]
function gmres_handle(ws::GmresWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}(); Vp = basis_ptrs(ws.V)
    ck(ccall((:khip_gmres_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Ptr{Cdouble}}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, length(ws.c), ws.x.ptr, ws.w.ptr, Vp, r))
    ck(ccall((:khip_gmres_workspace_set_grow, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), r[], GROW_VECTOR[], pointer_from_objref(ws)))
    h = r[]
    finalizer(_ -> ccall((:khip_gmres_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
# khip_grow_fn: restart = false lets the basis outgrow `memory` -- push!(V, similar(x)), src/gmres.jl:319-324
function grow_vector(ud::Ptr{Cvoid})::Ptr{Cdouble}
  ws = unsafe_pointer_to_objref(ud)::GmresWs
  t0 = time_ns()
  v = try similar(ws.x) catch; return Ptr{Cdouble}(C_NULL) end
  push!(ws.V, v)
  ws.stats.allocation_timer += (time_ns() - t0) / 1e9
  return v.ptr
end
const GROW_VECTOR = Ref{Ptr{Cvoid}}(C_NULL)
gmres_adopt(h, name, v::HIPVector) = ck(ccall((:khip_gmres_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

function Krylov.gmres!(ws::GmresWs, A::HIPCsr, b::HIPVector; M = I, N = I, ldiv::Bool = false, restart::Bool = false,
                       reorthogonalization::Bool = false, atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0,
                       timemax::Float64 = Inf, verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout,
                       fused::Int = 2)
  if ldiv || !native_precond(M) || !native_precond(N) || !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.gmres!, Tuple{GmresWs,Any,AbstractVector{Float64}}, ws, A, b; M, N, ldiv, restart, reorthogonalization, atol, rtol, itmax,
                  timemax, verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :128-140
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  m == n || error("System must be square")
  length(b) == m || error("Inconsistent problem size")
  Krylov.allocate_if(M !== I, ws, :q, HIPVector, ws.x)                                       # :142-144
  Krylov.allocate_if(N !== I, ws, :p, HIPVector, ws.x)
  Krylov.allocate_if(restart, ws, :Δx, HIPVector, ws.x)
  h = gmres_handle(ws)
  for (name, v) in (("x", ws.x), ("w", ws.w), ("p", ws.p), ("q", ws.q), ("dx", ws.Δx))
    gmres_adopt(h, name, v)
  end
  Vp = basis_ptrs(ws.V)                                                                     # the basis as it is now (it may have grown)
  ck(ccall((:khip_gmres_workspace_adopt_basis, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Cdouble}}), h, length(Vp), Vp))
  ws.warm_start && ck(ccall((:khip_gmres_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, ws.Δx.ptr))
  sp = ccall((:khip_gmres_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, restart, reorthogonalization, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  opA = Ref(Operator(A))
  rc = GC.@preserve ws A b M N opts opA box ccall((:khip_gmres_solve, lib), Cint, (Ptr{Cvoid}, Ref{Operator}, Ptr{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ref{Options}),
                                                   h, opA, opref(M), opref(N), b.ptr, opts)
  st = fill_stats!(ws.stats, sp, history)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_gmres_last_path, lib), Cint, (Ptr{Cvoid},), h)
  # the host fields of the workspace in the reference's own storage (c, s, z, packed R, inner_iter; src/krylov_workspaces.jl:2866-2871)
  len = Ref{Cint}(); inner = Ref{Cint}()
  ck(ccall((:khip_gmres_host_state, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cint}, Ref{Cint}),
           h, 0, C_NULL, C_NULL, C_NULL, C_NULL, len, inner))
  k = Int(len[]);  resize!(ws.c, k);  resize!(ws.s, k);  resize!(ws.z, k);  resize!(ws.R, div(k * (k + 1), 2))
  ck(ccall((:khip_gmres_host_state, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cint}, Ref{Cint}),
           h, k, ws.c, ws.s, ws.z, ws.R, len, inner))
  ws.inner_iter = inner[]
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ bicgstab!  (src/bicgstab.jl:125-277)
const BicgstabWs = BicgstabWorkspace{Float64,Float64,HIPVector}
function bicgstab_handle(ws::BicgstabWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_bicgstab_workspace_adopt, lib), Cint,
             (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.x.ptr, ws.r.ptr, ws.p.ptr, ws.v.ptr, ws.s.ptr, ws.qd.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_bicgstab_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
bicgstab_adopt(h, name, v::HIPVector) = ck(ccall((:khip_bicgstab_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

function Krylov.bicgstab!(ws::BicgstabWs, A::HIPCsr, b::HIPVector; c::HIPVector = b, M = I, N = I, ldiv::Bool = false,
                          atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0, timemax::Float64 = Inf,
                          verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  if ldiv || !native_precond(M) || !native_precond(N) || !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.bicgstab!, Tuple{BicgstabWs,Any,AbstractVector{Float64}}, ws, A, b; c, M, N, ldiv, atol, rtol, itmax, timemax, verbose, history,
                  callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :132-143
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  m == n || error("System must be square")
  length(b) == m || error("Inconsistent problem size")
  Krylov.allocate_if(M !== I, ws, :t, HIPVector, ws.x)                                       # :148-149
  Krylov.allocate_if(N !== I, ws, :yz, HIPVector, ws.x)
  h = bicgstab_handle(ws)
  for (name, v) in (("x", ws.x), ("r", ws.r), ("p", ws.p), ("v", ws.v), ("s", ws.s), ("qd", ws.qd), ("yz", ws.yz), ("t", ws.t), ("dx", ws.Δx))
    bicgstab_adopt(h, name, v)
  end
  ws.warm_start && ck(ccall((:khip_bicgstab_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, ws.Δx.ptr))
  sp = ccall((:khip_bicgstab_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  opA = Ref(Operator(A))
  rc = GC.@preserve ws A b c M N opts opA box ccall((:khip_bicgstab_solve, lib), Cint,
                                                 (Ptr{Cvoid}, Ref{Operator}, Ptr{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Options}),
                                                 h, opA, opref(M), opref(N), b.ptr, c.ptr, opts)
  st = fill_stats!(ws.stats, sp, history)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_bicgstab_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ minres!  (src/minres.jl:164-484)
struct MinresParams                 # khip_minres_params: λ, etol, conlim
  lambda::Cdouble; etol::Cdouble; conlim::Cdouble
end
const MinresWs = MinresWorkspace{Float64,Float64,HIPVector}
function minres_handle(ws::MinresWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_minres_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                        Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, length(ws.err_vec), ws.x.ptr, ws.r1.ptr, ws.r2.ptr, ws.w1.ptr, ws.w2.ptr, ws.y.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_minres_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
minres_adopt(h, name, v::HIPVector) = ck(ccall((:khip_minres_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

function Krylov.minres!(ws::MinresWs, A::HIPCsr, b::HIPVector; M = I, ldiv::Bool = false, linesearch::Bool = false, λ::Float64 = 0.0,
                        atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), etol::Float64 = √eps(Float64),
                        conlim::Float64 = 1/√eps(Float64), itmax::Int = 0, timemax::Float64 = Inf, verbose::Int = 0,
                        history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  if ldiv || linesearch || !native_precond(M) || !native_log(verbose, iostream)     # linesearch: nonpositive curvature is generic-only
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.minres!, Tuple{MinresWs,Any,AbstractVector{Float64}}, ws, A, b; M, ldiv, linesearch, λ, atol, rtol, etol, conlim,
                  itmax, timemax, verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # the reference's own argument checks, :172-179
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  m == n || error("System must be square")
  length(b) == n || error("Inconsistent problem size")
  Krylov.allocate_if(M !== I, ws, :v, HIPVector, ws.x)                                        # :192
  h = minres_handle(ws)
  for (name, v) in (("v", ws.v), ("npc_dir", ws.npc_dir), ("dx", ws.Δx))
    minres_adopt(h, name, v)
  end
  ws.warm_start && ck(ccall((:khip_minres_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, ws.Δx.ptr))
  sp = ccall((:khip_minres_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  prm = Ref(MinresParams(λ, etol, conlim))
  opA = Ref(Operator(A))
  rc = GC.@preserve ws A b M opts prm opA box ccall((:khip_minres_solve, lib), Cint,
                                                     (Ptr{Cvoid}, Ref{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid}),
                                                     h, opA, opref(M), b.ptr, opts, prm)
  st = fill_stats!(ws.stats, sp, history)
  if history                                                                                # stats.Aresiduals, stats.Acond
    ar, nar, ac, nac = Ref{Ptr{Cvoid}}(), Ref{Cint}(0), Ref{Ptr{Cvoid}}(), Ref{Cint}(0)
    ck(ccall((:khip_minres_histories, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Cint}, Ref{Ptr{Cvoid}}, Ref{Cint}), h, ar, nar, ac, nac))
    nar[] > 0 && append!(ws.stats.Aresiduals, unsafe_wrap(Array, Ptr{Float64}(ar[]), Int(nar[])))
    nac[] > 0 && append!(ws.stats.Acond, unsafe_wrap(Array, Ptr{Float64}(ac[]), Int(nac[])))
  end
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_minres_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ minres_qlp!  (src/minres_qlp.jl:131-538)
struct MinresQlpParams              # khip_minres_qlp_params: λ, Artol
  lambda::Cdouble; Artol::Cdouble
end
const MinresQlpWs = MinresQlpWorkspace{Float64,Float64,HIPVector}
function minres_qlp_handle(ws::MinresQlpWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_minres_qlp_workspace_adopt, lib), Cint,
             (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.x.ptr, ws.wₖ₋₁.ptr, ws.wₖ.ptr, ws.M⁻¹vₖ₋₁.ptr, ws.M⁻¹vₖ.ptr, ws.p.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_minres_qlp_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
minres_qlp_adopt(h, name, v::HIPVector) = ck(ccall((:khip_minres_qlp_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

# The fused loops rotate the roles of (M⁻¹vₖ₋₁, M⁻¹vₖ, p) and swap those of (wₖ₋₁, wₖ): after the solve only x and the stats are defined
# on this side.  linesearch (nonpositive curvature, npc_dir) is the generic method's.
function Krylov.minres_qlp!(ws::MinresQlpWs, A::HIPCsr, b::HIPVector; M = I, ldiv::Bool = false, linesearch::Bool = false, λ::Float64 = 0.0,
                            atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), Artol::Float64 = √eps(Float64),
                            itmax::Int = 0, timemax::Float64 = Inf, verbose::Int = 0, history::Bool = false, callback = nothing,
                            iostream::IO = Krylov.kstdout, fused::Int = 2)
  if ldiv || linesearch || !native_precond(M) || !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.minres_qlp!, Tuple{MinresQlpWs,Any,AbstractVector{Float64}}, ws, A, b; M, ldiv, linesearch, λ, atol, rtol, Artol,
                  itmax, timemax, verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :137-140
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  m == n || error("System must be square")
  length(b) == m || error("Inconsistent problem size")
  Krylov.allocate_if(M !== I, ws, :vₖ, HIPVector, ws.x)                                       # :152
  h = minres_qlp_handle(ws)
  for (name, v) in (("vk", ws.vₖ), ("dx", ws.Δx))
    minres_qlp_adopt(h, name, v)
  end
  ws.warm_start && ck(ccall((:khip_minres_qlp_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, ws.Δx.ptr))
  sp = ccall((:khip_minres_qlp_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  prm = Ref(MinresQlpParams(λ, Artol))
  opA = Ref(Operator(A))
  rc = GC.@preserve ws A b M opts prm opA box ccall((:khip_minres_qlp_solve, lib), Cint,
                                                     (Ptr{Cvoid}, Ref{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid}),
                                                     h, opA, opref(M), b.ptr, opts, prm)
  st = fill_stats!(ws.stats, sp, history)
  if history                                                                                # stats.Aresiduals, stats.Acond
    ar, nar, ac, nac = Ref{Ptr{Cvoid}}(), Ref{Cint}(0), Ref{Ptr{Cvoid}}(), Ref{Cint}(0)
    ck(ccall((:khip_minres_qlp_histories, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Cint}, Ref{Ptr{Cvoid}}, Ref{Cint}), h, ar, nar, ac, nac))
    nar[] > 0 && append!(ws.stats.Aresiduals, unsafe_wrap(Array, Ptr{Float64}(ar[]), Int(nar[])))
    nac[] > 0 && append!(ws.stats.Acond, unsafe_wrap(Array, Ptr{Float64}(ac[]), Int(nac[])))
  end
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_minres_qlp_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ bilq!  (src/bilq.jl:118-407)
struct BilqParams                   # khip_bilq_params: transfer_to_bicg, the adjoints of M and N (NULL: the operator itself)
  transfer_to_bicg::Cint; Mt::Ptr{Operator}; Nt::Ptr{Operator}
end
const BilqWs = BilqWorkspace{Float64,Float64,HIPVector}
function bilq_handle(ws::BilqWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_bilq_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                      Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.uₖ₋₁.ptr, ws.uₖ.ptr, ws.q.ptr, ws.vₖ₋₁.ptr, ws.vₖ.ptr, ws.p.ptr, ws.x.ptr, ws.d̅.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_bilq_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
self_adjoint_precond(M) = M === I || (M isa HIPOperator && M.kind === :jacobi)
bilq_adopt(h, name, v::HIPVector) = ck(ccall((:khip_bilq_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

# The adjoint is `A'`, built once per matrix and cached in `A.adj` (Base.adjoint above).  M and N are I or the library's Jacobi
# operator (diagonal: its own adjoint, so Mt = Nt = NULL is right).  ILU(0) of a nonsymmetric A is NOT its own adjoint and the
# library has no transposed solve: it is refused rather than run as N A' M in place of N' A' M'.
# After the solve only ws.x and ws.stats are defined: the library rotates the roles of (vₖ₋₁, vₖ) and (uₖ₋₁, uₖ) among the adopted vectors instead of copying them.
function Krylov.bilq!(ws::BilqWs, A::HIPCsr, b::HIPVector; c::HIPVector = b, transfer_to_bicg::Bool = true, M = I, N = I, ldiv::Bool = false,
                      atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0, timemax::Float64 = Inf,
                      verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  for (name, P) in (("M", M), ("N", N))
    (P isa HIPOperator && P.kind !== :jacobi) &&
      error("bilq!: $name = $(P.kind) is not its own adjoint and its transposed solve is not available: use I or KrylovHIP.jacobi(A)")
  end
  if ldiv || !self_adjoint_precond(M) || !self_adjoint_precond(N) || !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.bilq!, Tuple{BilqWs,Any,AbstractVector{Float64}}, ws, A, b; c, transfer_to_bicg, M, N, ldiv, atol, rtol, itmax, timemax,
                  verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :124-127
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  m == n || error("System must be square")
  length(b) == m || error("Inconsistent problem size")
  Krylov.allocate_if(M !== I, ws, :t, HIPVector, ws.x)                                       # :145-146
  Krylov.allocate_if(N !== I, ws, :s, HIPVector, ws.x)
  At = A'
  h = bilq_handle(ws)
  for (name, v) in (("t", ws.t), ("s", ws.s), ("dx", ws.Δx))
    bilq_adopt(h, name, v)
  end
  ws.warm_start && ck(ccall((:khip_bilq_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, ws.Δx.ptr))
  sp = ccall((:khip_bilq_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  prm = Ref(BilqParams(transfer_to_bicg, C_NULL, C_NULL))
  opA = Ref(Operator(A));  opAt = Ref(Operator(At))
  rc = GC.@preserve ws A At b c M N opts prm opA opAt box ccall((:khip_bilq_solve, lib), Cint,
         (Ptr{Cvoid}, Ref{Operator}, Ref{Operator}, Ptr{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid}),
         h, opA, opAt, opref(M), opref(N), b.ptr, c.ptr, opts, prm)
  st = fill_stats!(ws.stats, sp, history)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_bilq_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ qmr!  (src/qmr.jl:124-406)
struct QmrParams                    # khip_qmr_params: the adjoints of M and N (NULL: the operator itself)
  Mt::Ptr{Operator}; Nt::Ptr{Operator}
end
const QmrWs = QmrWorkspace{Float64,Float64,HIPVector}
function qmr_handle(ws::QmrWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_qmr_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.uₖ₋₁.ptr, ws.uₖ.ptr, ws.q.ptr, ws.vₖ₋₁.ptr, ws.vₖ.ptr, ws.p.ptr, ws.x.ptr, ws.wₖ₋₂.ptr, ws.wₖ₋₁.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_qmr_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
qmr_adopt(h, name, v::HIPVector) = ck(ccall((:khip_qmr_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

# As for bilq!: the adjoint is `A'`, built once per matrix and cached in `A.adj`; M and N are I or the library's Jacobi operator
# (its own adjoint, so Mt = Nt = NULL is right); ILU(0) is refused rather than run as N A' M in place of N' A' M'.
# After the solve only ws.x and ws.stats are defined: the library rotates the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and (wₖ₋₂, wₖ₋₁) among the adopted vectors.
function Krylov.qmr!(ws::QmrWs, A::HIPCsr, b::HIPVector; c::HIPVector = b, M = I, N = I, ldiv::Bool = false,
                     atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0, timemax::Float64 = Inf,
                     verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  for (name, P) in (("M", M), ("N", N))
    (P isa HIPOperator && P.kind !== :jacobi) &&
      error("qmr!: $name = $(P.kind) is not its own adjoint and its transposed solve is not available: use I or KrylovHIP.jacobi(A)")
  end
  if ldiv || !self_adjoint_precond(M) || !self_adjoint_precond(N) || !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.qmr!, Tuple{QmrWs,Any,AbstractVector{Float64}}, ws, A, b; c, M, N, ldiv, atol, rtol, itmax, timemax,
                  verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :130-133
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  m == n || error("System must be square")
  length(b) == m || error("Inconsistent problem size")
  Krylov.allocate_if(M !== I, ws, :t, HIPVector, ws.x)                                       # :151-152
  Krylov.allocate_if(N !== I, ws, :s, HIPVector, ws.x)
  At = A'
  h = qmr_handle(ws)
  for (name, v) in (("t", ws.t), ("s", ws.s), ("dx", ws.Δx))
    qmr_adopt(h, name, v)
  end
  ws.warm_start && ck(ccall((:khip_qmr_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, ws.Δx.ptr))
  sp = ccall((:khip_qmr_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  prm = Ref(QmrParams(C_NULL, C_NULL))
  opA = Ref(Operator(A));  opAt = Ref(Operator(At))
  rc = GC.@preserve ws A At b c M N opts prm opA opAt box ccall((:khip_qmr_solve, lib), Cint,
         (Ptr{Cvoid}, Ref{Operator}, Ref{Operator}, Ptr{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid}),
         h, opA, opAt, opref(M), opref(N), b.ptr, c.ptr, opts, prm)
  st = fill_stats!(ws.stats, sp, history)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_qmr_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ usymqr!  (src/usymqr.jl:130-365)
const UsymqrWs = UsymqrWorkspace{Float64,Float64,HIPVector,HIPVector}
function usymqr_handle(ws::UsymqrWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_usymqr_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                        Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.vₖ₋₁.ptr, ws.vₖ.ptr, ws.q.ptr, ws.x.ptr, ws.wₖ₋₂.ptr, ws.wₖ₋₁.ptr, ws.uₖ₋₁.ptr, ws.uₖ.ptr, ws.p.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_usymqr_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
usymqr_adopt(h, name, v::HIPVector) = ck(ccall((:khip_usymqr_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

# A has m rows and n columns; b has m entries, c has n.  The adjoint is `A'`, built once per matrix and cached in `A.adj`.  A
# rectangular system runs the library's primitive sequence (LAST_PATH[] == 0) whatever `fused` says.  After the solve only ws.x and
# ws.stats are defined: the library rotates the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and (wₖ₋₂, wₖ₋₁) among the adopted vectors.
function Krylov.usymqr!(ws::UsymqrWs, A::HIPCsr, b::HIPVector, c::HIPVector;
                        atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0, timemax::Float64 = Inf,
                        verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  if !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.usymqr!, Tuple{UsymqrWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c; atol, rtol, itmax, timemax,
                  verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :133-136
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  length(b) == m || error("Inconsistent problem size")
  length(c) == n || error("Inconsistent problem size")
  At = A'
  h = usymqr_handle(ws)
  usymqr_adopt(h, "dx", ws.Δx)
  ws.warm_start && ck(ccall((:khip_usymqr_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, ws.Δx.ptr))
  sp = ccall((:khip_usymqr_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  opA = Ref(Operator(A));  opAt = Ref(Operator(At))
  rc = GC.@preserve ws A At b c opts opA opAt box ccall((:khip_usymqr_solve, lib), Cint,
         (Ptr{Cvoid}, Ref{Operator}, Ref{Operator}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Options}),
         h, opA, opAt, b.ptr, c.ptr, opts)
  st = fill_stats!(ws.stats, sp, history)
  if history                                                                                # stats.Aresiduals
    ar, nar = Ref{Ptr{Cvoid}}(), Ref{Cint}(0)
    ck(ccall((:khip_usymqr_aresiduals, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Cint}), h, ar, nar))
    nar[] > 0 && append!(ws.stats.Aresiduals, unsafe_wrap(Array, Ptr{Float64}(ar[]), Int(nar[])))
  end
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_usymqr_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ usymlq!  (src/usymlq.jl:124-366)
struct UsymlqParams                # khip_usymlq_params: transfer_to_usymcg
  transfer_to_usymcg::Cint
end
const UsymlqWs = UsymlqWorkspace{Float64,Float64,HIPVector,HIPVector}
function usymlq_handle(ws::UsymlqWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_usymlq_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                        Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.uₖ₋₁.ptr, ws.uₖ.ptr, ws.p.ptr, ws.x.ptr, ws.d̅.ptr, ws.vₖ₋₁.ptr, ws.vₖ.ptr, ws.q.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_usymlq_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
usymlq_adopt(h, name, v::HIPVector) = ck(ccall((:khip_usymlq_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

# A has m rows and n columns; b has m entries, c has n.  The adjoint is `A'`, built once per matrix and cached in `A.adj`.  A
# rectangular system runs the library's primitive sequence (LAST_PATH[] == 0) whatever `fused` says.  After the solve only ws.x and
# ws.stats are defined: the library rotates the roles of (vₖ₋₁, vₖ) and (uₖ₋₁, uₖ) among the adopted vectors.
function Krylov.usymlq!(ws::UsymlqWs, A::HIPCsr, b::HIPVector, c::HIPVector; transfer_to_usymcg::Bool = true,
                        atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0, timemax::Float64 = Inf,
                        verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  if !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.usymlq!, Tuple{UsymlqWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c; transfer_to_usymcg, atol,
                  rtol, itmax, timemax, verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :130-133
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  length(b) == m || error("Inconsistent problem size")
  length(c) == n || error("Inconsistent problem size")
  At = A'
  h = usymlq_handle(ws)
  usymlq_adopt(h, "dx", ws.Δx)
  ws.warm_start && ck(ccall((:khip_usymlq_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, ws.Δx.ptr))
  sp = ccall((:khip_usymlq_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  prm = Ref(UsymlqParams(Cint(transfer_to_usymcg)))
  opA = Ref(Operator(A));  opAt = Ref(Operator(At))
  rc = GC.@preserve ws A At b c opts prm opA opAt box ccall((:khip_usymlq_solve, lib), Cint,
         (Ptr{Cvoid}, Ref{Operator}, Ref{Operator}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid}),
         h, opA, opAt, b.ptr, c.ptr, opts, prm)
  st = fill_stats!(ws.stats, sp, history)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_usymlq_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ trilqr!  (src/trilqr.jl:115-460)
struct TrilqrParams                # khip_trilqr_params: transfer_to_usymcg
  transfer_to_usymcg::Cint
end
const TrilqrWs = TrilqrWorkspace{Float64,Float64,HIPVector,HIPVector}
function trilqr_handle(ws::TrilqrWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_trilqr_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                        Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                        Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.uₖ₋₁.ptr, ws.uₖ.ptr, ws.p.ptr, ws.d̅.ptr, ws.x.ptr, ws.vₖ₋₁.ptr, ws.vₖ.ptr, ws.q.ptr, ws.y.ptr, ws.wₖ₋₃.ptr, ws.wₖ₋₂.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_trilqr_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
trilqr_adopt(h, name, v::HIPVector) = ck(ccall((:khip_trilqr_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))
# AdjointStats from khip_trilqr_adjoint_stats: both histories, both flags and the FULL status (khip_stats.status[96] cannot hold four
# of the reference's strings); niter and timer from khip_stats.  (khip_stats.inconsistent, the dual side's flag, has no field there.)
function fill_trilqr_stats!(stats::Krylov.AdjointStats{Float64}, h::Ptr{Cvoid}, sp::Ptr{Stats}, history::Bool)
  st = unsafe_load(sp)
  sprim, sdual, np, nd = Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0)
  rp, rd, status = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
  ck(ccall((:khip_trilqr_adjoint_stats, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Ptr{Cvoid}}, Ref{Cint}, Ref{Ptr{Cvoid}},
                                                     Ref{Cint}, Ref{Ptr{Cvoid}}), h, sprim, sdual, rp, np, rd, nd, status))
  Krylov.reset!(stats)
  history && np[] > 0 && append!(stats.residuals_primal, unsafe_wrap(Array, Ptr{Float64}(rp[]), Int(np[])))
  history && nd[] > 0 && append!(stats.residuals_dual, unsafe_wrap(Array, Ptr{Float64}(rd[]), Int(nd[])))
  stats.niter = st.niter;  stats.solved_primal = sprim[] != 0;  stats.solved_dual = sdual[] != 0
  stats.timer = st.timer;  stats.status = unsafe_string(Ptr{UInt8}(status[]))
  return st
end
# a user's callback reads both histories: they are brought over before it runs (the shared trampoline knows stats.residuals only)
trilqr_callback(cb, h, sp, history) = cb === nothing ? nothing : (w -> (fill_trilqr_stats!(w.stats, h, sp, history); cb(w)))

# A has m rows and n columns; b has m entries, c has n.  The adjoint is `A'`, built once per matrix and cached in `A.adj`.  trilqr!
# has no M or N.  A rectangular system runs the library's primitive sequence (LAST_PATH[] == 0) whatever `fused` says.  After the
# solve only ws.x, ws.y and ws.stats are defined: the library rotates the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and (wₖ₋₃, wₖ₋₂) among the
# adopted vectors.
function Krylov.trilqr!(ws::TrilqrWs, A::HIPCsr, b::HIPVector, c::HIPVector; transfer_to_usymcg::Bool = true,
                        atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0, timemax::Float64 = Inf,
                        verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  if !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.trilqr!, Tuple{TrilqrWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c; transfer_to_usymcg, atol,
                  rtol, itmax, timemax, verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :121-124
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  length(b) == m || error("Inconsistent problem size")
  length(c) == n || error("Inconsistent problem size")
  At = A'
  h = trilqr_handle(ws)
  for (name, v) in (("dx", ws.Δx), ("dy", ws.Δy))
    trilqr_adopt(h, name, v)
  end
  ws.warm_start && ck(ccall((:khip_trilqr_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, ws.Δx.ptr, ws.Δy.ptr))
  sp = ccall((:khip_trilqr_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(trilqr_callback(user_callback(callback), h, sp, history), ws, sp, false)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  prm = Ref(TrilqrParams(Cint(transfer_to_usymcg)))
  opA = Ref(Operator(A));  opAt = Ref(Operator(At))
  rc = GC.@preserve ws A At b c opts prm opA opAt box ccall((:khip_trilqr_solve, lib), Cint,
         (Ptr{Cvoid}, Ref{Operator}, Ref{Operator}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid}),
         h, opA, opAt, b.ptr, c.ptr, opts, prm)
  st = fill_trilqr_stats!(ws.stats, h, sp, history)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_trilqr_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ tricg!  (src/tricg.jl:149-484)
struct TricgParams                 # khip_tricg_params: τ, ν, spd, snd, flip
  tau::Cdouble
  nu::Cdouble
  spd::Cint
  snd::Cint
  flip::Cint
end
const TricgWs = TricgWorkspace{Float64,Float64,HIPVector,HIPVector}
function tricg_handle(ws::TricgWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_tricg_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                       Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                       Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.y.ptr, ws.N⁻¹uₖ₋₁.ptr, ws.N⁻¹uₖ.ptr, ws.p.ptr, ws.gy₂ₖ₋₁.ptr, ws.gy₂ₖ.ptr, ws.x.ptr, ws.M⁻¹vₖ₋₁.ptr, ws.M⁻¹vₖ.ptr, ws.q.ptr, ws.gx₂ₖ₋₁.ptr, ws.gx₂ₖ.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_tricg_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
tricg_adopt(h, name, v::HIPVector) = ck(ccall((:khip_tricg_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

# A has m rows and n columns; b and x have m entries, c and y have n.  The adjoint is `A'`, built once per matrix and cached in
# `A.adj`.  M and N other than I take the generic method (the library has M = N = I only).  A rectangular system runs the library's
# primitive sequence (LAST_PATH[] == 0) whatever `fused` says.  After the solve only ws.x, ws.y and ws.stats are defined: the library
# rotates the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ), (gx₂ₖ₋₁, gx₂ₖ) and (gy₂ₖ₋₁, gy₂ₖ) among the adopted vectors.
function Krylov.tricg!(ws::TricgWs, A::HIPCsr, b::HIPVector, c::HIPVector; M = I, N = I, ldiv::Bool = false, spd::Bool = false,
                       snd::Bool = false, flip::Bool = false, τ::Float64 = 1.0, ν::Float64 = -1.0, atol::Float64 = √eps(Float64),
                       rtol::Float64 = √eps(Float64), itmax::Int = 0, timemax::Float64 = Inf, verbose::Int = 0, history::Bool = false,
                       callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  if !native_log(verbose, iostream) || !(M === I) || !(N === I)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.tricg!, Tuple{TricgWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c; M, N, ldiv, spd, snd, flip,
                  τ, ν, atol, rtol, itmax, timemax, verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :155-158
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  length(b) == m || error("Inconsistent problem size")
  length(c) == n || error("Inconsistent problem size")
  At = A'
  h = tricg_handle(ws)
  for (name, v) in (("dx", ws.Δx), ("dy", ws.Δy))
    tricg_adopt(h, name, v)
  end
  ws.warm_start && ck(ccall((:khip_tricg_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, ws.Δx.ptr, ws.Δy.ptr))
  sp = ccall((:khip_tricg_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  prm = Ref(TricgParams(τ, ν, Cint(spd), Cint(snd), Cint(flip)))
  opA = Ref(Operator(A));  opAt = Ref(Operator(At))
  rc = GC.@preserve ws A At b c opts prm opA opAt box ccall((:khip_tricg_solve, lib), Cint,
         (Ptr{Cvoid}, Ref{Operator}, Ref{Operator}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid}),
         h, opA, opAt, b.ptr, c.ptr, opts, prm)
  st = fill_stats!(ws.stats, sp, history)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_tricg_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ trimr!  (src/trimr.jl:150-577)
struct TrimrParams                 # khip_trimr_params: τ, ν, spd, snd, flip, sp
  tau::Cdouble
  nu::Cdouble
  spd::Cint
  snd::Cint
  flip::Cint
  sp::Cint
end
const TrimrWs = TrimrWorkspace{Float64,Float64,HIPVector,HIPVector}
function trimr_handle(ws::TrimrWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_trimr_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                       Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                       Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                       Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.y.ptr, ws.N⁻¹uₖ₋₁.ptr, ws.N⁻¹uₖ.ptr, ws.p.ptr, ws.gy₂ₖ₋₃.ptr, ws.gy₂ₖ₋₂.ptr, ws.gy₂ₖ₋₁.ptr, ws.gy₂ₖ.ptr, ws.x.ptr, ws.M⁻¹vₖ₋₁.ptr, ws.M⁻¹vₖ.ptr, ws.q.ptr, ws.gx₂ₖ₋₃.ptr, ws.gx₂ₖ₋₂.ptr, ws.gx₂ₖ₋₁.ptr, ws.gx₂ₖ.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_trimr_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
trimr_adopt(h, name, v::HIPVector) = ck(ccall((:khip_trimr_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

# A has m rows and n columns; b and x have m entries, c and y have n.  The adjoint is `A'`, built once per matrix and cached in
# `A.adj`.  M and N other than I take the generic method (the library has M = N = I only).  A rectangular system runs the library's
# primitive sequence (LAST_PATH[] == 0) whatever `fused` says.  After the solve only ws.x, ws.y and ws.stats are defined: the library
# rotates the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and of the pairs (g₂ₖ₋₃, g₂ₖ₋₂) and (g₂ₖ₋₁, g₂ₖ) of each side among the adopted vectors.
function Krylov.trimr!(ws::TrimrWs, A::HIPCsr, b::HIPVector, c::HIPVector; M = I, N = I, ldiv::Bool = false, spd::Bool = false,
                       snd::Bool = false, flip::Bool = false, sp::Bool = false, τ::Float64 = 1.0, ν::Float64 = -1.0, atol::Float64 = √eps(Float64),
                       rtol::Float64 = √eps(Float64), itmax::Int = 0, timemax::Float64 = Inf, verbose::Int = 0, history::Bool = false,
                       callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  if !native_log(verbose, iostream) || !(M === I) || !(N === I)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.trimr!, Tuple{TrimrWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c; M, N, ldiv, spd, snd, flip,
                  sp, τ, ν, atol, rtol, itmax, timemax, verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :156-159
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  length(b) == m || error("Inconsistent problem size")
  length(c) == n || error("Inconsistent problem size")
  At = A'
  h = trimr_handle(ws)
  for (name, v) in (("dx", ws.Δx), ("dy", ws.Δy))
    trimr_adopt(h, name, v)
  end
  ws.warm_start && ck(ccall((:khip_trimr_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, ws.Δx.ptr, ws.Δy.ptr))
  stp = ccall((:khip_trimr_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)    # (`sp` is the saddle-point keyword here)
  cbf, cbd, box = callback_args(user_callback(callback), ws, stp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  prm = Ref(TrimrParams(τ, ν, Cint(spd), Cint(snd), Cint(flip), Cint(sp)))
  opA = Ref(Operator(A));  opAt = Ref(Operator(At))
  rc = GC.@preserve ws A At b c opts prm opA opAt box ccall((:khip_trimr_solve, lib), Cint,
         (Ptr{Cvoid}, Ref{Operator}, Ref{Operator}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid}),
         h, opA, opAt, b.ptr, c.ptr, opts, prm)
  st = fill_stats!(ws.stats, stp, history)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_trimr_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ usymlqr!  (src/usymlqr.jl:136-509)
struct UsymlqrParams               # khip_usymlqr_params: ls, ln
  ls::Cint
  ln::Cint
end
const UsymlqrWs = UsymlqrWorkspace{Float64,Float64,HIPVector,HIPVector}
function usymlqr_handle(ws::UsymlqrWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_usymlqr_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                         Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                         Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.r.ptr, ws.x.ptr, ws.y.ptr, ws.z.ptr, ws.vₖ₋₁.ptr, ws.vₖ.ptr, ws.uₖ₋₁.ptr, ws.uₖ.ptr, ws.p.ptr, ws.q.ptr, ws.d̅.ptr, ws.wₖ₋₂.ptr, ws.wₖ₋₁.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_usymlqr_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
usymlqr_adopt(h, name, v::HIPVector) = ck(ccall((:khip_usymlqr_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

# A has m rows and n columns; b and x have m entries, c and y have n.  The adjoint is `A'`, built once per matrix and cached in
# `A.adj`.  `ldiv` has no meaning without preconditioners and is dropped.  A rectangular system runs the library's primitive
# sequence (LAST_PATH[] == 0) whatever `fused` says.  After the solve only ws.x, ws.y and ws.stats are defined: the library rotates
# the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and (wₖ₋₂, wₖ₋₁) among the adopted vectors.
function Krylov.usymlqr!(ws::UsymlqrWs, A::HIPCsr, b::HIPVector, c::HIPVector; ls::Bool = true, ln::Bool = true, ldiv::Bool = false,
                         atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0, timemax::Float64 = Inf,
                         verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  if !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.usymlqr!, Tuple{UsymlqrWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c; ls, ln, ldiv, atol,
                  rtol, itmax, timemax, verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :141-145
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  length(b) == m || error("Inconsistent problem size")
  length(c) == n || error("Inconsistent problem size")
  (ls || ln) || error("The keyword arguments `ls` and `ln` can't be both `false`.")
  At = A'
  h = usymlqr_handle(ws)
  for (name, v) in (("dx", ws.Δx), ("dy", ws.Δy))
    usymlqr_adopt(h, name, v)
  end
  ws.warm_start && ck(ccall((:khip_usymlqr_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, ws.Δx.ptr, ws.Δy.ptr))
  stp = ccall((:khip_usymlqr_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, stp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  prm = Ref(UsymlqrParams(Cint(ls), Cint(ln)))
  opA = Ref(Operator(A));  opAt = Ref(Operator(At))
  rc = GC.@preserve ws A At b c opts prm opA opAt box ccall((:khip_usymlqr_solve, lib), Cint,
         (Ptr{Cvoid}, Ref{Operator}, Ref{Operator}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid}),
         h, opA, opAt, b.ptr, c.ptr, opts, prm)
  st = fill_stats!(ws.stats, stp, history)
  if history                                                                                # stats.Aresiduals
    ar, nar = Ref{Ptr{Cvoid}}(), Ref{Cint}(0)
    ck(ccall((:khip_usymlqr_aresiduals, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Cint}), h, ar, nar))
    nar[] > 0 && append!(ws.stats.Aresiduals, unsafe_wrap(Array, Ptr{Float64}(ar[]), Int(nar[])))
  end
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_usymlqr_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ cgs!  (src/cgs.jl:126-281)
const CgsWs = CgsWorkspace{Float64,Float64,HIPVector}
function cgs_handle(ws::CgsWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_cgs_workspace_adopt, lib), Cint,
             (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.x.ptr, ws.r.ptr, ws.u.ptr, ws.p.ptr, ws.q.ptr, ws.ts.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_cgs_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
cgs_adopt(h, name, v::HIPVector) = ck(ccall((:khip_cgs_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

# Transpose-free: no A', and M and N are whatever the library applies (I, Jacobi, ILU(0)), as for bicgstab!.  The library rotates
# no roles: after the solve every vector of the workspace holds what the reference's variable of that name holds.
function Krylov.cgs!(ws::CgsWs, A::HIPCsr, b::HIPVector; c::HIPVector = b, M = I, N = I, ldiv::Bool = false,
                     atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0, timemax::Float64 = Inf,
                     verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  if ldiv || !native_precond(M) || !native_precond(N) || !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.cgs!, Tuple{CgsWs,Any,AbstractVector{Float64}}, ws, A, b; c, M, N, ldiv, atol, rtol, itmax, timemax,
                  verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :132-135
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  m == n || error("System must be square")
  length(b) == m || error("Inconsistent problem size")
  Krylov.allocate_if(M !== I, ws, :vw, HIPVector, ws.x)                                      # :148-149
  Krylov.allocate_if(N !== I, ws, :yz, HIPVector, ws.x)
  h = cgs_handle(ws)
  for (name, v) in (("vw", ws.vw), ("yz", ws.yz), ("dx", ws.Δx))
    cgs_adopt(h, name, v)
  end
  ws.warm_start && ck(ccall((:khip_cgs_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, ws.Δx.ptr))
  sp = ccall((:khip_cgs_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  opA = Ref(Operator(A))
  rc = GC.@preserve ws A b c M N opts opA box ccall((:khip_cgs_solve, lib), Cint,
                                                 (Ptr{Cvoid}, Ref{Operator}, Ptr{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Options}),
                                                 h, opA, opref(M), opref(N), b.ptr, c.ptr, opts)
  st = fill_stats!(ws.stats, sp, history)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_cgs_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ symmlq!  (src/symmlq.jl:132-464)
struct SymmlqParams                # khip_symmlq_params: λ, λest, etol, conlim, transfer_to_cg
  lambda::Cdouble; lambda_est::Cdouble; etol::Cdouble; conlim::Cdouble; transfer_to_cg::Cint
end
const SymmlqWs = SymmlqWorkspace{Float64,Float64,HIPVector}
function symmlq_handle(ws::SymmlqWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_symmlq_workspace_adopt, lib), Cint,
             (Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, length(ws.clist), ws.x.ptr, ws.Mvold.ptr, ws.Mv.ptr, ws.Mv_next.ptr, ws.w̅.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_symmlq_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
# SymmlqStats (src/krylov_stats.jl) has no inconsistent / indefinite / npcCount; reset! empties its four histories
function fill_stats!(stats::Krylov.SymmlqStats{Float64}, sp::Ptr{Stats}, history::Bool)
  st = unsafe_load(sp)
  Krylov.reset!(stats)
  history && st.nres > 0 && append!(stats.residuals, unsafe_wrap(Array, st.residuals, Int(st.nres)))
  stats.niter = st.niter;  stats.solved = st.solved != 0
  stats.timer = st.timer;  stats.status = cstr(st.status)
  return st
end
symmlq_adopt(h, name, v::HIPVector) =ck(ccall((:khip_symmlq_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))

# The window lists (clist, zlist, sprod) live in the library, which takes their length from ws.clist.  The fused loops rotate the
# roles of (Mvold, Mv, Mv_next): after the solve only x and the stats are defined on this side.  NaN in residualscg and errorscg is
# the reference's `missing`.
function Krylov.symmlq!(ws::SymmlqWs, A::HIPCsr, b::HIPVector; M = I, ldiv::Bool = false, transfer_to_cg::Bool = true, λ::Float64 = 0.0,
                        λest::Float64 = 0.0, atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64),
                        etol::Float64 = √eps(Float64), conlim::Float64 = 1/√eps(Float64), itmax::Int = 0, timemax::Float64 = Inf,
                        verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  if ldiv || !native_precond(M) || !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.symmlq!, Tuple{SymmlqWs,Any,AbstractVector{Float64}}, ws, A, b; M, ldiv, transfer_to_cg, λ, λest, atol, rtol,
                  etol, conlim, itmax, timemax, verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :138-141
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  m == n || error("System must be square")
  length(b) == m || error("Inconsistent problem size")
  Krylov.allocate_if(M !== I, ws, :v, HIPVector, ws.x)                                        # :152
  h = symmlq_handle(ws)
  for (name, v) in (("v", ws.v), ("dx", ws.Δx))
    symmlq_adopt(h, name, v)
  end
  ws.warm_start && ck(ccall((:khip_symmlq_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, ws.Δx.ptr))
  sp = ccall((:khip_symmlq_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  prm = Ref(SymmlqParams(λ, λest, etol, conlim, transfer_to_cg))
  opA = Ref(Operator(A))
  rc = GC.@preserve ws A b M opts prm opA box ccall((:khip_symmlq_solve, lib), Cint,
                                                     (Ptr{Cvoid}, Ref{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid}),
                                                     h, opA, opref(M), b.ptr, opts, prm)
  st = fill_stats!(ws.stats, sp, history)
  if history                                                                               # stats.residualscg, errors, errorscg
    rc_, nrc, er, ner, ec, nec = Ref{Ptr{Cvoid}}(), Ref{Cint}(0), Ref{Ptr{Cvoid}}(), Ref{Cint}(0), Ref{Ptr{Cvoid}}(), Ref{Cint}(0)
    ck(ccall((:khip_symmlq_histories, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Cint}, Ref{Ptr{Cvoid}}, Ref{Cint}, Ref{Ptr{Cvoid}}, Ref{Cint}),
             h, rc_, nrc, er, ner, ec, nec))
    unmissing(v) = isnan(v) ? missing : v
    nrc[] > 0 && append!(ws.stats.residualscg, unmissing.(unsafe_wrap(Array, Ptr{Float64}(rc_[]), Int(nrc[]))))
    ner[] > 0 && append!(ws.stats.errors, unsafe_wrap(Array, Ptr{Float64}(er[]), Int(ner[])))
    nec[] > 0 && append!(ws.stats.errorscg, unmissing.(unsafe_wrap(Array, Ptr{Float64}(ec[]), Int(nec[]))))
  end
  an, ac = Ref{Cdouble}(NaN), Ref{Cdouble}(NaN)
  ck(ccall((:khip_symmlq_norms, lib), Cint, (Ptr{Cvoid}, Ref{Cdouble}, Ref{Cdouble}), h, an, ac))
  ws.stats.Anorm = an[];  ws.stats.Acond = ac[]
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_symmlq_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ bilqr!  (src/bilqr.jl:116-484)
struct BilqrParams                 # khip_bilqr_params: transfer_to_bicg
  transfer_to_bicg::Cint
end
const BilqrWs = BilqrWorkspace{Float64,Float64,HIPVector}
function bilqr_handle(ws::BilqrWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    ck(ccall((:khip_bilqr_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                       Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                       Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.uₖ₋₁.ptr, ws.uₖ.ptr, ws.q.ptr, ws.vₖ₋₁.ptr, ws.vₖ.ptr, ws.p.ptr, ws.x.ptr, ws.y.ptr, ws.d̅.ptr, ws.wₖ₋₃.ptr, ws.wₖ₋₂.ptr, r))
    h = r[]
    finalizer(_ -> ccall((:khip_bilqr_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
bilqr_adopt(h, name, v::HIPVector) = ck(ccall((:khip_bilqr_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, dptr(v)))
# AdjointStats from khip_bilqr_adjoint_stats: both histories, both flags and the FULL status (khip_stats.status[96] cannot hold four
# of the reference's strings); niter and timer from khip_stats
function fill_adjoint_stats!(stats::Krylov.AdjointStats{Float64}, h::Ptr{Cvoid}, sp::Ptr{Stats}, history::Bool)
  st = unsafe_load(sp)
  sprim, sdual, np, nd = Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0)
  rp, rd, status = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
  ck(ccall((:khip_bilqr_adjoint_stats, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Ptr{Cvoid}}, Ref{Cint}, Ref{Ptr{Cvoid}},
                                                    Ref{Cint}, Ref{Ptr{Cvoid}}), h, sprim, sdual, rp, np, rd, nd, status))
  Krylov.reset!(stats)
  history && np[] > 0 && append!(stats.residuals_primal, unsafe_wrap(Array, Ptr{Float64}(rp[]), Int(np[])))
  history && nd[] > 0 && append!(stats.residuals_dual, unsafe_wrap(Array, Ptr{Float64}(rd[]), Int(nd[])))
  stats.niter = st.niter;  stats.solved_primal = sprim[] != 0;  stats.solved_dual = sdual[] != 0
  stats.timer = st.timer;  stats.status = unsafe_string(Ptr{UInt8}(status[]))
  return st
end
# a user's callback reads both histories: they are brought over before it runs (the shared trampoline knows stats.residuals only)
bilqr_callback(cb, h, sp, history) = cb === nothing ? nothing : (w -> (fill_adjoint_stats!(w.stats, h, sp, history); cb(w)))

# The adjoint is `A'`, built once per matrix and cached in `A.adj`.  bilqr! has no M or N.  After the solve only ws.x, ws.y and
# ws.stats are defined: the library rotates the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and (wₖ₋₃, wₖ₋₂) among the adopted vectors.
function Krylov.bilqr!(ws::BilqrWs, A::HIPCsr, b::HIPVector, c::HIPVector; transfer_to_bicg::Bool = true,
                       atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0, timemax::Float64 = Inf,
                       verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout, fused::Int = 2)
  if !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.bilqr!, Tuple{BilqrWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c; transfer_to_bicg, atol, rtol,
                  itmax, timemax, verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # :122-126
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  m == n || error("Systems must be square")
  length(b) == m || error("Inconsistent problem size")
  length(c) == n || error("Inconsistent problem size")
  At = A'
  h = bilqr_handle(ws)
  for (name, v) in (("dx", ws.Δx), ("dy", ws.Δy))
    bilqr_adopt(h, name, v)
  end
  ws.warm_start && ck(ccall((:khip_bilqr_warm_start, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), h, ws.Δx.ptr, ws.Δy.ptr))
  sp = ccall((:khip_bilqr_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(bilqr_callback(user_callback(callback), h, sp, history), ws, sp, false)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  prm = Ref(BilqrParams(transfer_to_bicg))
  opA = Ref(Operator(A));  opAt = Ref(Operator(At))
  rc = GC.@preserve ws A At b c opts prm opA opAt box ccall((:khip_bilqr_solve, lib), Cint,
         (Ptr{Cvoid}, Ref{Operator}, Ref{Operator}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid}),
         h, opA, opAt, b.ptr, c.ptr, opts, prm)
  st = fill_adjoint_stats!(ws.stats, h, sp, history)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_bilqr_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ cg_lanczos_shift!  (src/cg_lanczos_shift.jl:107-284)
struct LanczosShiftParams           # khip_cg_lanczos_shift_params: shifts (host array), nshifts, check_curvature
  shifts::Ptr{Cdouble}; nshifts::Cint; check_curvature::Cint
end
const CgLanczosShiftWs = CgLanczosShiftWorkspace{Float64,Float64,HIPVector}
function cg_lanczos_shift_handle(ws::CgLanczosShiftWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}()
    xs = Ptr{Cdouble}[v.ptr for v in ws.x];  ps = Ptr{Cdouble}[v.ptr for v in ws.p]
    ck(ccall((:khip_cg_lanczos_shift_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                                                   Ptr{Ptr{Cdouble}}, Ptr{Ptr{Cdouble}}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.nshifts, ws.Mv.ptr, ws.Mv_prev.ptr, ws.Mv_next.ptr, xs, ps, r))
    h = r[]
    finalizer(_ -> ccall((:khip_cg_lanczos_shift_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
# stats.residuals[i], stats.indefinite and the workspace's per-shift arrays from the library (after the solve and before every callback)
function sync_shift_state!(ws::CgLanczosShiftWs, h::Ptr{Cvoid}, history::Bool)
  p = ws.nshifts
  a = Vector{Float64}(undef, 8p)
  ck(ccall((:khip_cg_lanczos_shift_arrays, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, a))
  for (k, dst) in enumerate((ws.rNorms, ws.σ, ws.δhat, ws.ω, ws.γ))
    dst .= view(a, (k - 1) * p + 1:k * p)
  end
  for (k, dst) in enumerate((ws.converged, ws.not_cv, ws.stats.indefinite))
    dst .= view(a, (4 + k) * p + 1:(5 + k) * p) .!= 0
  end
  for i in 1:p
    empty!(ws.stats.residuals[i])
    history || continue
    ptr, cnt = Ref{Ptr{Cvoid}}(), Ref{Cint}(0)
    ck(ccall((:khip_cg_lanczos_shift_residuals, lib), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}, Ref{Cint}), h, i - 1, ptr, cnt))
    cnt[] > 0 && append!(ws.stats.residuals[i], unsafe_wrap(Array, Ptr{Float64}(ptr[]), Int(cnt[])))
  end
  return ws
end

function Krylov.cg_lanczos_shift!(ws::CgLanczosShiftWs, A::HIPCsr, b::HIPVector, shifts::AbstractVector{Float64}; M = I, ldiv::Bool = false,
                                  check_curvature::Bool = false, atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0,
                                  timemax::Float64 = Inf, verbose::Int = 0, history::Bool = false, callback = nothing,
                                  iostream::IO = Krylov.kstdout, fused::Int = 2)
  if ldiv || !native_precond(M) || !native_log(verbose, iostream)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.cg_lanczos_shift!, Tuple{CgLanczosShiftWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, shifts;
                  M, ldiv, check_curvature, atol, rtol, itmax, timemax, verbose, history,
                  callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, n = size(A)                                                                            # the reference's own argument checks, :115-122
  (m == ws.m && n == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $n)")
  m == n || error("System must be square")
  length(b) == n || error("Inconsistent problem size")
  nshifts = length(shifts)
  nshifts == ws.nshifts || error("workspace.nshifts = $(ws.nshifts) is inconsistent with length(shifts) = $nshifts")
  Krylov.allocate_if(M !== I, ws, :v, HIPVector, ws.Mv)                                      # :133
  h = cg_lanczos_shift_handle(ws)
  ck(ccall((:khip_cg_lanczos_shift_workspace_adopt_vector, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, "v", dptr(ws.v)))
  sp = ccall((:khip_cg_lanczos_shift_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cb = user_callback(callback)
  # the callback reads ws.x, ws.stats and the per-shift arrays: they are brought over before it runs (the loop is host-driven then)
  cbw = cb === nothing ? nothing : (w -> (sync_shift_state!(w, h, history); cb(w)))
  cbf, cbd, box = callback_args(cbw, ws, sp, false)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, fused, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  sh = Vector{Float64}(shifts)
  prm = Ref(LanczosShiftParams(pointer(sh), Cint(nshifts), Cint(check_curvature)))
  opA = Ref(Operator(A))
  rc = GC.@preserve ws A b M sh opts prm opA box ccall((:khip_cg_lanczos_shift_solve, lib), Cint,
                                                        (Ptr{Cvoid}, Ref{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid}),
                                                        h, opA, opref(M), b.ptr, opts, prm)
  st = unsafe_load(sp)
  sync_shift_state!(ws, h, history)
  ws.stats.niter = st.niter;  ws.stats.solved = st.solved != 0;  ws.stats.timer = st.timer;  ws.stats.status = cstr(st.status)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_cg_lanczos_shift_last_path, lib), Cint, (Ptr{Cvoid},), h)
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

# ------------------------------------------------------------------------------------------------ device matrix (block solvers)
# Tall blocks are libkrylov_hip panels (ROW-major, rows padded to 16, padding rows zero), small blocks host matrices -- exactly
# where the library keeps them (csrc/block.cpp) and where the reference's own small LAPACK calls run.  INTEGRATION.md has the
# line-by-line table of what block_gmres! asks of its matrix type.
mutable struct HIPMatrix <: AbstractMatrix{Float64}
  ptr::Ptr{Float64}; host::Union{Nothing,Matrix{Float64}}; m::Int; k::Int
  function HIPMatrix(::UndefInitializer, m::Integer, k::Integer)
    m <= 4k && return new(C_NULL, Matrix{Float64}(undef, m, k), m, k)              # Z, C, D, R, H and the (0, 0) placeholders
    np = Ref{Int64}(); ck(ccall((:khip_panel_rows, lib), Cint, (Int64, Ref{Int64}), m, np))
    r = Ref{Ptr{Cvoid}}(C_NULL); ck(ccall((:khip_malloc, lib), Cint, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), CTX[].h, 8np[] * k, r))
    A = new(Ptr{Float64}(r[]), nothing, m, k)
    ck(ccall((:khip_fill, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Cdouble), CTX[].h, np[] * k, A.ptr, 0.0))   # padding rows stay zero
    finalizer(x -> ccall((:khip_free, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), CTX[].h, x.ptr), A)
  end
end
tall(A::HIPMatrix) = A.host === nothing
plen(A::HIPMatrix) = (np = Ref{Int64}(); ccall((:khip_panel_rows, lib), Cint, (Int64, Ref{Int64}), A.m, np); np[] * A.k)
Base.size(A::HIPMatrix) = (A.m, A.k)
Base.isempty(A::HIPMatrix) = A.m == 0 || A.k == 0
Base.getindex(A::HIPMatrix, i...) = tall(A) ? error("scalar indexing of a device panel") : A.host[i...]
Base.setindex!(A::HIPMatrix, v, i...) = (A.host[i...] = v)                       # H[k][1:p,:] .= R, small blocks only
Base.view(A::HIPMatrix, I...) = view(A.host, I...)                               # D1 = view(D, 1:p, :)
Krylov.ktypeof(::HIPMatrix) = HIPMatrix
Krylov.matrix_to_vector(::Type{HIPMatrix}) = Vector{Float64}                    # tau, buffer: host
function HIPMatrix(B::Matrix{Float64}); A = HIPMatrix(undef, size(B)...); tall(A) || (A.host .= B; return A)
  t = HIPVector(vec(B)); ck(ccall((:khip_panel_from_colmajor, lib), Cint, (Ptr{Cvoid}, Int64, Cint, Ptr{Cdouble}, Ptr{Cdouble}), CTX[].h, A.m, A.k, t.ptr, A.ptr)); A; end
function Base.Matrix(A::HIPMatrix); tall(A) || return copy(A.host)
  t = HIPVector(undef, A.m * A.k); ck(ccall((:khip_panel_to_colmajor, lib), Cint, (Ptr{Cvoid}, Int64, Cint, Ptr{Cdouble}, Ptr{Cdouble}), CTX[].h, A.m, A.k, A.ptr, t.ptr))
  reshape(Vector(t), A.m, A.k); end
Base.fill!(A::HIPMatrix, v) = tall(A) ? (ck(ccall((:khip_fill, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Cdouble), CTX[].h, plen(A), A.ptr, v)); A) : (fill!(A.host, v); A)
Krylov.kfill!(A::HIPMatrix, v) = fill!(A, v)
Base.copyto!(D::HIPMatrix, S::HIPMatrix) = tall(D) ? (ck(ccall((:khip_copy, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}), CTX[].h, plen(D), D.ptr, S.ptr)); D) : (copyto!(D.host, S.host); D)
LinearAlgebra.norm(A::HIPMatrix) = tall(A) ? (r = Ref{Cdouble}(); ck(ccall((:khip_panel_norm, lib), Cint, (Ptr{Cvoid}, Int64, Cint, Ptr{Cdouble}, Ref{Cdouble}), CTX[].h, A.m, A.k, A.ptr, r)); r[]) : norm(A.host)
# the two panel broadcasts of the solver: W .= B .- W (:160, :207) and X .+= ΔX (:161, :331); small blocks broadcast as Matrix
Base.BroadcastStyle(::Type{HIPMatrix}) = Broadcast.ArrayStyle{HIPMatrix}()
function Base.copyto!(D::HIPMatrix, bc::Broadcast.Broadcasted{Broadcast.ArrayStyle{HIPMatrix}})
  tall(D) || (copyto!(D.host, Broadcast.Broadcasted(bc.f, map(a -> a isa HIPMatrix ? a.host : a, bc.args))); return D)
  a, b = bc.args
  if bc.f === (-) && b === D      # D .= a .- D
    ck(ccall((:khip_axpby, lib), Cint, (Ptr{Cvoid}, Int64, Cdouble, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}), CTX[].h, plen(D), 1.0, a.ptr, -1.0, D.ptr))
  elseif bc.f === (+) && a === D  # D .+= b
    ck(ccall((:khip_axpy, lib), Cint, (Ptr{Cvoid}, Int64, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}), CTX[].h, plen(D), 1.0, b.ptr, D.ptr))
  else error("panel broadcast not used by block_gmres!") end
  D
end
# products (:242, :245, :246, :325)
# (a system with n <= 4p keeps even X, W and V on the host: its products go column by column through the SpMV -- correctness only)
function LinearAlgebra.mul!(W::HIPMatrix, A::HIPCsr, P::HIPMatrix)
  if !tall(P)
    for j in 1:P.k; W.host[:, j] = Vector(kmul!(HIPVector(undef, A.m), A, HIPVector(P.host[:, j]))); end
    return W
  end
  ck(ccall((:khip_spmm, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint), CTX[].h, A.h, P.ptr, W.ptr, P.k)); W
end
function LinearAlgebra.mul!(Ψ::HIPMatrix, Vt::Adjoint{Float64,HIPMatrix}, Q::HIPMatrix)
  V = parent(Vt)
  tall(V) || return (mul!(Ψ.host, V.host', Q.host); Ψ)
  ck(ccall((:khip_panel_gemm_tn, lib), Cint, (Ptr{Cvoid}, Int64, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), CTX[].h, V.m, V.k, V.ptr, Q.ptr, Ψ.host)); Ψ
end
function LinearAlgebra.mul!(Q::HIPMatrix, V::HIPMatrix, Ψ::HIPMatrix, α::Number, β::Number)
  tall(Q) || return (mul!(Q.host, V.host, Ψ.host, α, β); Q)                      # Y[i] -= R[pos] Y[j]   (:317)
  ck(ccall((:khip_panel_gemm_nn, lib), Cint, (Ptr{Cvoid}, Int64, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}), CTX[].h, V.m, V.k, α, V.ptr, Ψ.host, β, Q.ptr)); Q
end
LinearAlgebra.ldiv!(U::UpperTriangular{Float64,HIPMatrix}, Y::HIPMatrix) = (ldiv!(UpperTriangular(parent(U).host), Y.host); Y)   # :320
Base.:*(A::HIPCsr, X::HIPMatrix) = mul!(HIPMatrix(undef, A.m, X.k), A, X)
# householder!(Q, R, tau, buffer; compact) (src/block_krylov_utils.jl:201-208): tall Q on the device, small H blocks with LAPACK.
# The workspace's `buffer` has length 0 for any SM that is not a `Matrix` (src/block_krylov_workspaces.jl:155-158), and the
# `Matrix{Float64}` methods taking a buffer pass lwork = length(buffer) to dgeqrf / dormqr and ignore `info`
# (src/block_krylov_utils.jl:230-236, :282-290): with lwork = 0 they would silently do nothing.  The small host blocks therefore
# go through the BUFFER-LESS forms (src/block_krylov_utils.jl:192-199 and the generic fallbacks :294-300 = LAPACK.geqrf! /
# orgqr! / ormqr!, which size their own workspace).
function Krylov.householder!(Q::HIPMatrix, R::HIPMatrix, τ::Vector{Float64}, buffer::Vector{Float64}; compact::Bool=false)
  if tall(Q)                       # kgeqrf! + copy_triangle + korgqr! in one call; same Q, R, tau as LAPACK
    ck(ccall((:khip_panel_qr_tau, lib), Cint, (Ptr{Cvoid}, Int64, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), CTX[].h, Q.m, Q.k, Q.ptr, R.host, τ))
  else
    Krylov.householder!(Q.host, R.host, τ; compact)          # 3-argument form: no (empty) buffer
  end
  Q, R
end
Krylov.kormqr!(side::Char, trans::Char, H::HIPMatrix, τ::Vector{Float64}, D::HIPMatrix, buffer::Vector{Float64}) = Krylov.kormqr!(side, trans, H.host, τ, D.host)   # :266, :279 -- 5-argument form

# ------------------------------------------------------------------------------------------------ block_gmres!  (src/block_gmres.jl:110-358)
const BlockGmresWs = BlockGmresWorkspace{Float64,Float64,Vector{Float64},HIPMatrix}
panel_ptrs(V::Vector{HIPMatrix}) = Ptr{Cdouble}[v.ptr for v in V]
pptr(A::HIPMatrix) = (isempty(A) || !tall(A)) ? Ptr{Cdouble}(C_NULL) : A.ptr
function block_gmres_handle(ws::BlockGmresWs)
  get!(HANDLES, ws) do
    r = Ref{Ptr{Cvoid}}(); Vp = panel_ptrs(ws.V)
    ck(ccall((:khip_block_gmres_workspace_adopt, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Ptr{Cdouble}}, Ref{Ptr{Cvoid}}),
             CTX[].h, ws.m, ws.n, ws.p, length(ws.V), ws.X.ptr, ws.W.ptr, Vp, r))
    ck(ccall((:khip_block_gmres_workspace_set_grow, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), r[], GROW_PANEL[], pointer_from_objref(ws)))
    h = r[]
    finalizer(_ -> ccall((:khip_block_gmres_workspace_destroy, lib), Cint, (Ptr{Cvoid},), h), ws)
    h
  end
end
function grow_panel(ud::Ptr{Cvoid})::Ptr{Cdouble}            # push!(V, SM(undef, n, p)), src/block_gmres.jl:300-305 (a zeroed panel)
  ws = unsafe_pointer_to_objref(ud)::BlockGmresWs
  t0 = time_ns()
  P = try HIPMatrix(undef, ws.n, ws.p) catch; return Ptr{Cdouble}(C_NULL) end
  push!(ws.V, P)
  ws.stats.allocation_timer += (time_ns() - t0) / 1e9
  return P.ptr
end
const GROW_PANEL = Ref{Ptr{Cvoid}}(C_NULL)
block_adopt(h, name, A::HIPMatrix) = ck(ccall((:khip_block_gmres_workspace_adopt_panel, lib), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), h, name, pptr(A)))

function Krylov.block_gmres!(ws::BlockGmresWs, A::HIPCsr, B::HIPMatrix; M = I, N = I, ldiv::Bool = false, restart::Bool = false,
                             reorthogonalization::Bool = false, atol::Float64 = √eps(Float64), rtol::Float64 = √eps(Float64), itmax::Int = 0,
                             timemax::Float64 = Inf, verbose::Int = 0, history::Bool = false, callback = nothing, iostream::IO = Krylov.kstdout)
  n, p = ws.n, ws.p
  # native loop: M = N = I (the block solver's preconditioners would be applied to panels), tall panels
  if ldiv || M !== I || N !== I || !native_log(verbose, iostream) || !tall(B) || !tall(ws.X)
    GENERIC_SOLVES[] += 1
    return invoke(Krylov.block_gmres!, Tuple{BlockGmresWs,Any,AbstractMatrix{Float64}}, ws, A, B; M, N, ldiv, restart, reorthogonalization, atol, rtol,
                  itmax, timemax, verbose, history, callback = callback === nothing ? (w -> false) : callback, iostream)
  end
  m, nA = size(A);  s, pB = size(B)                                                          # :117-128
  (m == ws.m && nA == ws.n) || error("(workspace.m, workspace.n) = ($(ws.m), $(ws.n)) is inconsistent with size(A) = ($m, $nA)")
  m == nA || error("System must be square")
  nA == s || error("Inconsistent problem size")
  pB == p || error("the workspace was built for $p right-hand sides, B has $pB")
  Krylov.allocate_if(restart, ws, :ΔX, HIPMatrix, n, p)                                       # :145
  h = block_gmres_handle(ws)
  for (name, P) in (("X", ws.X), ("W", ws.W), ("P", ws.P), ("Q", ws.Q), ("dX", ws.ΔX))
    block_adopt(h, name, P)
  end
  Vp = panel_ptrs(ws.V)
  ck(ccall((:khip_block_gmres_workspace_adopt_basis, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Cdouble}}), h, length(Vp), Vp))
  ws.warm_start && ck(ccall((:khip_block_gmres_warm_start_panel, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h, ws.ΔX.ptr))
  sp = ccall((:khip_block_gmres_stats, lib), Ptr{Stats}, (Ptr{Cvoid},), h)
  cbf, cbd, box = callback_args(user_callback(callback), ws, sp, history)
  opts = Ref(Options(; atol, rtol, itmax, timemax, history, restart, reorthogonalization, verbose, log_fd = logfd(iostream), callback = cbf, callback_data = cbd))
  opA = Ref(Operator(A))
  rc = GC.@preserve ws A B opts opA box ccall((:khip_block_gmres_solve_panel, lib), Cint,
                                           (Ptr{Cvoid}, Ref{Operator}, Ptr{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ref{Options}),
                                           h, opA, C_NULL, C_NULL, B.ptr, opts)
  st = fill_stats!(ws.stats, sp, history)
  NATIVE_SOLVES[] += 1;  LAST_PATH[] = ccall((:khip_block_gmres_last_path, lib), Cint, (Ptr{Cvoid},), h)
  ws.warm_start = false
  finish_callback(box)
  rc == 0 || failed(st)
  return ws
end

function __init__()
  GROW_VECTOR[] = @cfunction(grow_vector, Ptr{Cdouble}, (Ptr{Cvoid},))
  GROW_PANEL[] = @cfunction(grow_panel, Ptr{Cdouble}, (Ptr{Cvoid},))
  CALLBACK[] = @cfunction(callback_trampoline, Cint, (Ptr{Cvoid}, Ptr{Cvoid}))
  return nothing
end

end # module
