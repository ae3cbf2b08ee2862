# trilqr.jl -- trilqr! through the specialised method (the library's device-resident loop on A and A') against the generic method of
# Krylov.jl on the same device types.  Included from runtests.jl, and stand-alone beside it:
#
#   julia --project=julia/KrylovHIP julia/KrylovHIP/test/trilqr.jl     (needs an MI355X and krylov.jl_amd/libkrylov_hip.so)
using Test, LinearAlgebra, SparseArrays
using Krylov, KrylovHIP
import KrylovHIP: HIPVector, HIPCsr, CTX, Ctx

@isdefined(unsymmetric_breakdown) || include(joinpath(pkgdir(Krylov), "test", "test_utils.jl"))   # kron_unsymmetric, rectangular_adjoint, ...

if !@isdefined(native)                                               # stand-alone: runtests.jl has made the context and `native`
  CTX[] = Ctx(0)
  function native(body, path::Integer)
    n0 = KrylovHIP.NATIVE_SOLVES[]; g0 = KrylovHIP.GENERIC_SOLVES[]
    out = body()
    @test KrylovHIP.NATIVE_SOLVES[] == n0 + 1
    @test KrylovHIP.GENERIC_SOLVES[] == g0
    @test KrylovHIP.LAST_PATH[] == path
    out
  end
end
generic(f!, ws, A, b, c; kw...) = invoke(f!, Tuple{typeof(ws),Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c; kw...)

@testset "trilqr! -- KrylovHIP" begin
  A_cpu, b_cpu = kron_unsymmetric(7)
  A_cpu = sparse(A_cpu) + 24.0 * I                                   # the shifted operator: both sides converge in under 30 iterations
  n = size(A_cpu, 1)
  c_cpu = sin.(0.11 .* (0:n-1)) .+ 1.2
  A_gpu = HIPCsr(A_cpu)
  b = HIPVector(b_cpu)
  c = HIPVector(c_cpu)
  S = HIPVector

  @testset "trilqr(A_gpu, b_gpu, c_gpu)" begin
    x, t, stats = native(2) do; trilqr(A_gpu, b, c); end             # forwards callback = workspace -> false
    @test stats.solved_primal && stats.solved_dual
    @test norm(b_cpu - A_cpu * Vector(x)) ≤ 1e-6 * norm(b_cpu)
    @test norm(c_cpu - A_cpu' * Vector(t)) ≤ 1e-6 * norm(c_cpu)
    @test A_gpu' === A_gpu'                                          # A' is built once and kept on the matrix
  end

  @testset "native against generic" begin
    ws = TrilqrWorkspace(n, n, S, S); ws2 = TrilqrWorkspace(n, n, S, S)
    native(2) do; trilqr!(ws, A_gpu, b, c; history = true); end
    generic(trilqr!, ws2, A_gpu, b, c; history = true)
    @test ws.stats.niter == ws2.stats.niter
    @test ws.stats.status == ws2.stats.status == "Both primal and dual solutions (xᶜ, t) are good enough given atol and rtol"
    @test length(ws.stats.residuals_primal) == length(ws2.stats.residuals_primal)
    @test length(ws.stats.residuals_dual) == length(ws2.stats.residuals_dual)
    @test ws.stats.residuals_primal ≈ ws2.stats.residuals_primal rtol = 1e-5
    @test ws.stats.residuals_dual ≈ ws2.stats.residuals_dual rtol = 1e-5
    @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    @test Vector(ws.y) ≈ Vector(ws2.y) rtol = 1e-6
    for kw in ((itmax = 1,), (itmax = 2,), (itmax = 3,), (itmax = 4,), (itmax = 7,), (transfer_to_usymcg = false,))
      native(2) do; trilqr!(ws, A_gpu, b, c; kw...); end
      generic(trilqr!, ws2, A_gpu, b, c; kw...)
      @test ws.stats.niter == ws2.stats.niter
      @test ws.stats.status == ws2.stats.status
      @test (ws.stats.solved_primal, ws.stats.solved_dual) == (ws2.stats.solved_primal, ws2.stats.solved_dual)
      @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
      @test Vector(ws.y) ≈ Vector(ws2.y) rtol = 1e-6
    end
  end

  @testset "warm start, callback, verbose" begin
    ws = TrilqrWorkspace(n, n, S, S)
    x0 = HIPVector(collect(range(-0.5, 0.5; length = n)))
    y0 = HIPVector(collect(range(0.25, -0.25; length = n)))
    native(2) do; trilqr!(ws, A_gpu, b, c, x0, y0); end
    @test ws.stats.solved_primal && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    @test ws.stats.solved_dual && norm(c_cpu - A_cpu' * Vector(ws.y)) ≤ 1e-6 * norm(c_cpu)
    seen = Tuple{Int,Int}[]
    native(1) do
      trilqr!(ws, A_gpu, b, c; history = true,
              callback = w -> (push!(seen, (length(w.stats.residuals_primal), length(w.stats.residuals_dual))); length(seen) == 3))
    end
    @test seen == [(2, 2), (3, 3), (4, 4)]
    @test ws.stats.status == "user-requested exit"
    io = IOBuffer()                                                  # no file descriptor: the generic method prints
    g0 = KrylovHIP.GENERIC_SOLVES[]
    trilqr!(ws, A_gpu, b, c; verbose = 1, iostream = io)
    @test KrylovHIP.GENERIC_SOLVES[] == g0 + 1
    @test occursin("TRILQR: primal system of $n equations in $n variables", String(take!(io)))
  end

  @testset "rectangular adjoint systems and the breakdown system of the reference" begin
    Ar, br, cr = rectangular_adjoint()                               # 10 x 25: the dual system is inconsistent
    Ar = sparse(Matrix(Ar))
    mr, nr = size(Ar)
    ws = TrilqrWorkspace(mr, nr, S, S)
    native(0) do; trilqr!(ws, HIPCsr(Ar), HIPVector(br), HIPVector(cr)); end   # m ≠ n: the primitive sequence
    @test norm(br - Ar * Vector(ws.x)) ≤ 1e-6 * norm(br)
    s = cr - Ar' * Vector(ws.y)
    @test norm(Ar * s) ≤ 1e-6 * norm(Ar * cr)
    @test ws.stats.solved_primal && ws.stats.solved_dual
    Ab, bb, cb = unsymmetric_breakdown()                             # δbar₁ = 0: the transfer is skipped at k = 1
    ws = TrilqrWorkspace(2, 2, S, S)
    native(2) do; trilqr!(ws, HIPCsr(sparse(Matrix(Ab))), HIPVector(bb), HIPVector(cb)); end
    @test ws.stats.solved_primal && ws.stats.solved_dual
    @test norm(bb - Ab * Vector(ws.x)) ≤ 1e-6 * norm(bb)
    @test norm(cb - Ab' * Vector(ws.y)) ≤ 1e-6 * norm(cb)
  end
end
