# bilqr.jl -- bilqr! through the specialised method (the library's device-resident loop on A and A', one Lanczos process for the
# primal and the dual system) against the generic method of Krylov.jl on the same device types.  Included from runtests.jl, and
# stand-alone beside it:
#
#   julia --project=julia/KrylovHIP julia/KrylovHIP/test/bilqr.jl      (needs an MI355X and krylov.jl_amd/libkrylov_hip.so)
using Test, LinearAlgebra, SparseArrays
using Krylov, KrylovHIP
import KrylovHIP: HIPVector, HIPCsr, CTX, Ctx

@isdefined(kron_unsymmetric) || include(joinpath(pkgdir(Krylov), "test", "test_utils.jl"))   # kron_unsymmetric, unsymmetric_breakdown, bc_breakdown

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
generic_bilqr(ws, A, b, c; kw...) = invoke(bilqr!, Tuple{typeof(ws),Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c; kw...)

@testset "bilqr! -- KrylovHIP" begin
  A_cpu, b_cpu = kron_unsymmetric(8)
  A_cpu = sparse(A_cpu)
  n = size(A_cpu, 1)
  c_cpu = sin.(0.11 .* (0:n-1)) .+ 1.2
  A_gpu = HIPCsr(A_cpu)
  b = HIPVector(b_cpu)
  c = HIPVector(c_cpu)
  S = HIPVector

  @testset "bilqr(A_gpu, b_gpu, c_gpu)" begin
    x, y, stats = native(2) do; bilqr(A_gpu, b, c); end               # forwards callback = workspace -> false
    @test stats.solved_primal && stats.solved_dual
    @test norm(b_cpu - A_cpu * Vector(x)) ≤ 1e-6 * norm(b_cpu)
    @test norm(c_cpu - A_cpu' * Vector(y)) ≤ 1e-6 * norm(c_cpu)
    @test A_gpu' === A_gpu'                                          # A' is built once and kept on the matrix
  end

  @testset "native against generic" begin
    ws = BilqrWorkspace(n, n, S); ws2 = BilqrWorkspace(n, n, S)
    native(2) do; bilqr!(ws, A_gpu, b, c; history = true); end
    generic_bilqr(ws2, A_gpu, b, c; history = true)
    @test ws.stats.niter == ws2.stats.niter
    @test ws.stats.status == ws2.stats.status
    @test ws.stats.solved_primal == ws2.stats.solved_primal && ws.stats.solved_dual == ws2.stats.solved_dual
    @test length(ws.stats.residuals_primal) == length(ws2.stats.residuals_primal)
    @test length(ws.stats.residuals_dual) == length(ws2.stats.residuals_dual)
    @test ws.stats.residuals_primal ≈ ws2.stats.residuals_primal rtol = 1e-5
    @test ws.stats.residuals_dual ≈ ws2.stats.residuals_dual rtol = 1e-5
    @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    @test Vector(ws.y) ≈ Vector(ws2.y) rtol = 1e-6
    for kw in ((transfer_to_bicg = false,), (itmax = 1,), (itmax = 2,), (itmax = 3,), (itmax = 4,), (itmax = 7,))
      native(2) do; bilqr!(ws, A_gpu, b, c; kw...); end
      generic_bilqr(ws2, A_gpu, b, c; kw...)
      @test ws.stats.niter == ws2.stats.niter
      @test ws.stats.status == ws2.stats.status
      @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
      @test Vector(ws.y) ≈ Vector(ws2.y) rtol = 1e-6
    end
  end

  @testset "warm start, callback, verbose" begin
    ws = BilqrWorkspace(n, n, S)
    x0 = HIPVector(collect(range(-0.5, 0.5; length = n)))
    y0 = HIPVector(collect(range(0.3, -0.2; length = n)))
    native(2) do; bilqr!(ws, A_gpu, b, c, x0, y0); end
    @test ws.stats.solved_primal && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    @test ws.stats.solved_dual && norm(c_cpu - A_cpu' * Vector(ws.y)) ≤ 1e-6 * norm(c_cpu)
    seen = Tuple{Int,Int}[]
    native(1) do
      bilqr!(ws, A_gpu, b, c; history = true,
             callback = w -> (push!(seen, (length(w.stats.residuals_primal), length(w.stats.residuals_dual))); length(seen) == 3))
    end
    @test seen == [(2, 2), (3, 3), (4, 4)]
    @test ws.stats.status == "user-requested exit"
    io = IOBuffer()                                                  # no file descriptor: the generic method prints
    g0 = KrylovHIP.GENERIC_SOLVES[]
    bilqr!(ws, A_gpu, b, c; verbose = 1, iostream = io)
    @test KrylovHIP.GENERIC_SOLVES[] == g0 + 1
    @test occursin("BILQR: systems of size $n", String(take!(io)))
  end

  @testset "the reference's breakdowns" begin
    A2, b2, c2 = unsymmetric_breakdown()
    ws = BilqrWorkspace(2, 2, S)
    native(2) do; bilqr!(ws, HIPCsr(sparse(A2)), HIPVector(b2), HIPVector(c2); history = true); end
    @test ws.stats.niter == 2 && !ws.stats.solved_primal && !ws.stats.solved_dual
    @test ws.stats.status == "Breakdown ⟨uₖ₊₁,vₖ₊₁⟩ = 0"
    @test Vector(ws.x) ≈ [0.0, 1.0] atol = 1e-12
    @test ws.stats.residuals_dual ≈ [1.0, 1.0, √2] atol = 1e-12
    @test isnan(ws.stats.residuals_primal[3])
    A3, b3, c3 = bc_breakdown()
    bilqr!(ws, HIPCsr(sparse(A3)), HIPVector(b3), HIPVector(c3))
    @test ws.stats.niter == 0 && !ws.stats.solved_primal && !ws.stats.solved_dual
    @test ws.stats.status == "Breakdown bᴴc = 0"
  end

  @testset "a status longer than khip_stats.status" begin            # diag(1, 2): 107 bytes, handed over whole
    ws = BilqrWorkspace(2, 2, S)
    bilqr!(ws, HIPCsr(sparse([1.0 0.0; 0.0 2.0])), HIPVector([1.0, 1.0]), HIPVector([1.0, 2.0]))
    @test ws.stats.niter == 3 && ws.stats.solved_primal && ws.stats.solved_dual
    @test endswith(ws.stats.status, "given atol and rtol") && sizeof(ws.stats.status) > 95
  end
end
