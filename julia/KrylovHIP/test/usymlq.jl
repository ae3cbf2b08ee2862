# usymlq.jl -- usymlq! through the specialised method (the library's device-resident loop on A and A') against the generic method of
# Krylov.jl on the same device types.  Included from runtests.jl, and stand-alone beside it:
#
#   julia --project=julia/KrylovHIP julia/KrylovHIP/test/usymlq.jl     (needs an MI355X and krylov.jl_amd/libkrylov_hip.so)
using Test, LinearAlgebra, SparseArrays
using Krylov, KrylovHIP
import KrylovHIP: HIPVector, HIPCsr, CTX, Ctx

@isdefined(unsymmetric_breakdown) || include(joinpath(pkgdir(Krylov), "test", "test_utils.jl"))   # kron_unsymmetric, over_consistent, ...

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

@testset "usymlq! -- KrylovHIP" begin
  A_cpu, b_cpu = kron_unsymmetric(4)
  A_cpu = sparse(A_cpu)
  n = size(A_cpu, 1)
  c_cpu = sin.(0.11 .* (0:n-1)) .+ 1.2
  A_gpu = HIPCsr(A_cpu)
  b = HIPVector(b_cpu)
  c = HIPVector(c_cpu)
  S = HIPVector

  @testset "usymlq(A_gpu, b_gpu, c_gpu)" begin
    x, stats = native(2) do; usymlq(A_gpu, b, c); end                # forwards callback = workspace -> false
    @test stats.solved
    @test norm(b_cpu - A_cpu * Vector(x)) ≤ 1e-6 * norm(b_cpu)
    @test A_gpu' === A_gpu'                                          # A' is built once and kept on the matrix
  end

  @testset "native against generic" begin
    ws = UsymlqWorkspace(n, n, S, S); ws2 = UsymlqWorkspace(n, n, S, S)
    native(2) do; usymlq!(ws, A_gpu, b, c; history = true); end
    generic(usymlq!, ws2, A_gpu, b, c; history = true)
    @test ws.stats.niter == ws2.stats.niter
    @test ws.stats.status == ws2.stats.status == "solution xᶜ good enough given atol and rtol"
    @test length(ws.stats.residuals) == ws.stats.niter + 1
    @test ws.stats.residuals ≈ ws2.stats.residuals rtol = 1e-5
    @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    @test Krylov.solution(ws) === ws.x
    for kw in ((itmax = 1,), (itmax = 2,), (itmax = 7,), (transfer_to_usymcg = false, itmax = 40))
      native(2) do; usymlq!(ws, A_gpu, b, c; kw...); end
      generic(usymlq!, ws2, A_gpu, b, c; kw...)
      @test ws.stats.niter == ws2.stats.niter
      @test ws.stats.status == ws2.stats.status
      @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    end
  end

  @testset "warm start, callback, verbose" begin
    ws = UsymlqWorkspace(n, n, S, S)
    x0 = HIPVector(collect(range(-0.5, 0.5; length = n)))
    native(2) do; usymlq!(ws, A_gpu, b, c, x0); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    seen = Int[]
    native(1) do
      usymlq!(ws, A_gpu, b, c; history = true, callback = w -> (push!(seen, length(w.stats.residuals)); length(seen) == 3))
    end
    @test seen == [2, 3, 4]
    @test ws.stats.status == "user-requested exit"
    io = IOBuffer()                                                  # no file descriptor: the generic method prints
    g0 = KrylovHIP.GENERIC_SOLVES[]
    usymlq!(ws, A_gpu, b, c; verbose = 1, iostream = io)
    @test KrylovHIP.GENERIC_SOLVES[] == g0 + 1
    @test occursin("USYMLQ: system of $n equations in $n variables", String(take!(io)))
  end

  @testset "rectangular systems and the breakdown system of the reference" begin
    for (sys, cvec) in ((over_consistent, ones(10)), (under_consistent, ones(25)), (square_consistent, ones(10)))
      Ar, br = sys()
      Ar = sparse(Matrix(Ar))
      mr, nr = size(Ar)
      ws = UsymlqWorkspace(mr, nr, S, S)
      native(mr == nr ? 2 : 0) do; usymlq!(ws, HIPCsr(Ar), HIPVector(br), HIPVector(cvec)); end   # m ≠ n: the primitive sequence
      @test norm(br - Ar * Vector(ws.x)) ≤ 1e-6 * norm(br)
      @test !ws.stats.inconsistent
    end
    Ab, bb, cb = unsymmetric_breakdown()                             # δbar₁ = 0: the transfer is skipped at k = 1
    ws = UsymlqWorkspace(2, 2, S, S)
    native(2) do; usymlq!(ws, HIPCsr(sparse(Matrix(Ab))), HIPVector(bb), HIPVector(cb)); end
    @test ws.stats.solved && ws.stats.niter == 2
    @test norm(bb - Ab * Vector(ws.x)) ≤ 1e-6 * norm(bb)
  end
end
