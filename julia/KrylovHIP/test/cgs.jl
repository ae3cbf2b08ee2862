# cgs.jl -- cgs! through the specialised method (the library's device-resident loop, transpose-free) against the generic method of
# Krylov.jl on the same device types.  Included from runtests.jl, and stand-alone beside it:
#
#   julia --project=julia/KrylovHIP julia/KrylovHIP/test/cgs.jl        (needs an MI355X and krylov.jl_amd/libkrylov_hip.so)
using Test, LinearAlgebra, SparseArrays
using Krylov, KrylovHIP
import KrylovHIP: HIPVector, HIPCsr, CTX, Ctx

@isdefined(kron_unsymmetric) || include(joinpath(pkgdir(Krylov), "test", "test_utils.jl"))   # kron_unsymmetric, bc_breakdown

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
generic_cgs(ws, A, b; kw...) = invoke(cgs!, Tuple{typeof(ws),Any,AbstractVector{Float64}}, ws, A, b; kw...)

@testset "cgs! -- KrylovHIP" begin
  A_cpu, b_cpu = kron_unsymmetric(8)
  A_cpu = sparse(A_cpu)
  n = size(A_cpu, 1)
  A_gpu = HIPCsr(A_cpu)
  b = HIPVector(b_cpu)
  S = HIPVector

  @testset "cgs(A_gpu, b_gpu)" begin
    x, stats = native(2) do; cgs(A_gpu, b); end                      # forwards callback = workspace -> false
    @test stats.solved
    @test norm(b_cpu - A_cpu * Vector(x)) ≤ 1e-6 * norm(b_cpu)
  end

  @testset "native against generic" begin
    ws = CgsWorkspace(n, n, S); ws2 = CgsWorkspace(n, n, S)
    native(2) do; cgs!(ws, A_gpu, b; history = true); end
    generic_cgs(ws2, A_gpu, b; history = true)
    @test ws.stats.niter == ws2.stats.niter
    @test ws.stats.status == ws2.stats.status
    @test length(ws.stats.residuals) == ws.stats.niter + 1
    @test ws.stats.residuals ≈ ws2.stats.residuals rtol = 1e-5
    @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    @test Krylov.solution(ws) === ws.x
    for kw in ((c = HIPVector(-b_cpu),), (itmax = 1,), (itmax = 3,))
      native(2) do; cgs!(ws, A_gpu, b; kw...); end
      generic_cgs(ws2, A_gpu, b; kw...)
      @test ws.stats.niter == ws2.stats.niter
      @test ws.stats.status == ws2.stats.status
      @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
      for f in (:u, :p, :q, :r)                                      # no role is rotated: the fields hold the reference's variables
        @test Vector(getfield(ws, f)) ≈ Vector(getfield(ws2, f)) rtol = 1e-6
      end
    end
  end

  @testset "warm start, Jacobi, callback, verbose" begin
    ws = CgsWorkspace(n, n, S)
    x0 = HIPVector(collect(range(-0.5, 0.5; length = n)))
    native(2) do; cgs!(ws, A_gpu, b, x0); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    native(1) do; cgs!(ws, A_gpu, b; M = KrylovHIP.jacobi(A_gpu)); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    native(1) do; cgs!(ws, A_gpu, b; N = KrylovHIP.jacobi(A_gpu)); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    seen = Int[]
    native(1) do; cgs!(ws, A_gpu, b; history = true, callback = w -> (push!(seen, length(w.stats.residuals)); length(seen) == 3)); end
    @test seen == [2, 3, 4]
    @test ws.stats.status == "user-requested exit"
    io = IOBuffer()                                                  # no file descriptor: the generic method prints
    g0 = KrylovHIP.GENERIC_SOLVES[]
    cgs!(ws, A_gpu, b; verbose = 1, iostream = io)
    @test KrylovHIP.GENERIC_SOLVES[] == g0 + 1
    @test occursin("CGS: system of size $n", String(take!(io)))
  end

  @testset "breakdowns" begin
    A3, b3, c3 = bc_breakdown()
    ws = CgsWorkspace(2, 2, S)
    cgs!(ws, HIPCsr(sparse(A3)), HIPVector(b3); c = HIPVector(c3))
    @test ws.stats.niter == 0 && !ws.stats.solved
    @test ws.stats.status == "Breakdown bᴴc = 0"
    A2 = sparse([1.0 0.0; 1.0 2.0]);  e1 = [1.0, 0.0]                 # ρ₁ = 0 exactly, then σ₂ = 0: α₂ is NaN
    native(2) do; cgs!(ws, HIPCsr(A2), HIPVector(e1); history = true); end
    @test ws.stats.niter == 2 && !ws.stats.solved
    @test ws.stats.status == "breakdown αₖ == 0"
    @test ws.stats.residuals[1:2] == [1.0, 1.0] && isnan(ws.stats.residuals[3])
  end
end
