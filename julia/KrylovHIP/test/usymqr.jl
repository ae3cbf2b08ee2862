# usymqr.jl -- usymqr! through the specialised method (the library's device-resident loop on A and A') against the generic method of
# Krylov.jl on the same device types.  Included from runtests.jl, and stand-alone beside it:
#
#   julia --project=julia/KrylovHIP julia/KrylovHIP/test/usymqr.jl     (needs an MI355X and krylov.jl_amd/libkrylov_hip.so)
using Test, LinearAlgebra, SparseArrays
using Krylov, KrylovHIP
import KrylovHIP: HIPVector, HIPCsr, CTX, Ctx

@isdefined(over_inconsistent) || include(joinpath(pkgdir(Krylov), "test", "test_utils.jl"))   # kron_unsymmetric, over_consistent, ...

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

@testset "usymqr! -- KrylovHIP" begin
  A_cpu, b_cpu = kron_unsymmetric(4)
  A_cpu = sparse(A_cpu)
  n = size(A_cpu, 1)
  c_cpu = sin.(0.11 .* (0:n-1)) .+ 1.2
  A_gpu = HIPCsr(A_cpu)
  b = HIPVector(b_cpu)
  c = HIPVector(c_cpu)
  S = HIPVector

  @testset "usymqr(A_gpu, b_gpu, c_gpu)" begin
    x, stats = native(2) do; usymqr(A_gpu, b, c); end                # forwards callback = workspace -> false
    @test stats.solved
    @test norm(b_cpu - A_cpu * Vector(x)) ≤ 1e-6 * norm(b_cpu)
    @test A_gpu' === A_gpu'                                          # A' is built once and kept on the matrix
  end

  @testset "native against generic" begin
    ws = UsymqrWorkspace(n, n, S, S); ws2 = UsymqrWorkspace(n, n, S, S)
    native(2) do; usymqr!(ws, A_gpu, b, c; history = true); end
    generic(usymqr!, ws2, A_gpu, b, c; history = true)
    @test ws.stats.niter == ws2.stats.niter
    @test ws.stats.status == ws2.stats.status
    @test length(ws.stats.residuals) == ws.stats.niter + 1
    @test length(ws.stats.Aresiduals) == ws.stats.niter
    @test ws.stats.residuals ≈ ws2.stats.residuals rtol = 1e-5
    @test ws.stats.Aresiduals ≈ ws2.stats.Aresiduals rtol = 1e-5
    @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    @test Krylov.solution(ws) === ws.x
    for kw in ((itmax = 1,), (itmax = 2,), (itmax = 7,))
      native(2) do; usymqr!(ws, A_gpu, b, c; kw...); end
      generic(usymqr!, ws2, A_gpu, b, c; kw...)
      @test ws.stats.niter == ws2.stats.niter
      @test ws.stats.status == ws2.stats.status
      @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    end
  end

  @testset "warm start, callback, verbose" begin
    ws = UsymqrWorkspace(n, n, S, S)
    x0 = HIPVector(collect(range(-0.5, 0.5; length = n)))
    native(2) do; usymqr!(ws, A_gpu, b, c, x0); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    seen = Tuple{Int,Int}[]
    native(1) do
      usymqr!(ws, A_gpu, b, c; history = true,
              callback = w -> (push!(seen, (length(w.stats.residuals), length(w.stats.Aresiduals))); length(seen) == 3))
    end
    @test first.(seen) == [2, 3, 4]
    @test ws.stats.status == "user-requested exit"
    io = IOBuffer()                                                  # no file descriptor: the generic method prints
    g0 = KrylovHIP.GENERIC_SOLVES[]
    usymqr!(ws, A_gpu, b, c; verbose = 1, iostream = io)
    @test KrylovHIP.GENERIC_SOLVES[] == g0 + 1
    @test occursin("USYMQR: system of $n equations in $n variables", String(take!(io)))
  end

  @testset "rectangular and inconsistent systems of the reference" begin
    for (sys, cvec, flag) in ((over_consistent, ones(10), :solved), (under_consistent, ones(25), :solved),
                              (over_inconsistent, [2.0^i * (iseven(i) ? 1.0 : -1.0) for i = 1:10], :inconsistent),
                              (square_inconsistent, ones(10), :inconsistent))
      Ar, br = sys()
      Ar = sparse(Matrix(Ar))
      mr, nr = size(Ar)
      ws = UsymqrWorkspace(mr, nr, S, S)
      native(mr == nr ? 2 : 0) do; usymqr!(ws, HIPCsr(Ar), HIPVector(br), HIPVector(cvec)); end   # m ≠ n: the primitive sequence
      @test getfield(ws.stats, flag)
      flag === :solved && @test norm(br - Ar * Vector(ws.x)) ≤ 1e-6 * norm(br)
    end
  end
end
