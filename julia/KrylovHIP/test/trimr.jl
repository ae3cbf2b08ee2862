# trimr.jl -- trimr! through the specialised method (the library's device-resident loop on A and A') against the generic method of
# Krylov.jl on the same device types.  It does its own set-up: run it stand-alone, or include it after runtests.jl:
#
#   julia --project=julia/KrylovHIP julia/KrylovHIP/test/trimr.jl     (needs an MI355X and krylov.jl_amd/libkrylov_hip.so)
using Test, LinearAlgebra, SparseArrays
using Krylov, KrylovHIP
import KrylovHIP: HIPVector, HIPCsr, CTX, Ctx

@isdefined(ssy_mo_breakdown) || include(joinpath(pkgdir(Krylov), "test", "test_utils.jl"))   # kron_unsymmetric, small_sqd, ssy_mo_breakdown, ...

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
block_residual(A, b, c, x, y, τ, ν) = norm([b - τ * x - A * y; c - A' * x - ν * y]) / norm([b; c])

@testset "trimr! -- KrylovHIP" begin
  A_cpu, b_cpu = kron_unsymmetric(7)
  A_cpu = sparse(A_cpu) + 24.0 * I
  n = size(A_cpu, 1)
  c_cpu = sin.(0.11 .* (0:n-1)) .+ 1.2
  A_gpu = HIPCsr(A_cpu)
  b = HIPVector(b_cpu)
  c = HIPVector(c_cpu)
  S = HIPVector

  @testset "trimr(A_gpu, b_gpu, c_gpu)" begin
    x, y, stats = native(2) do; trimr(A_gpu, b, c); end              # forwards callback = workspace -> false, M = N = I
    @test stats.solved && !stats.inconsistent
    @test block_residual(A_cpu, b_cpu, c_cpu, Vector(x), Vector(y), 1.0, -1.0) ≤ 1e-6
    @test A_gpu' === A_gpu'                                          # A' is built once and kept on the matrix
  end

  @testset "native against generic" begin
    ws = TrimrWorkspace(n, n, S, S); ws2 = TrimrWorkspace(n, n, S, S)
    native(2) do; trimr!(ws, A_gpu, b, c; history = true); end
    generic(trimr!, ws2, A_gpu, b, c; history = true)
    @test ws.stats.niter == ws2.stats.niter
    @test ws.stats.status == ws2.stats.status == "solution good enough given atol and rtol"
    @test length(ws.stats.residuals) == length(ws2.stats.residuals)
    @test ws.stats.residuals ≈ ws2.stats.residuals rtol = 1e-5
    @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    @test Vector(ws.y) ≈ Vector(ws2.y) rtol = 1e-6
    for kw in ((itmax = 1,), (itmax = 2,), (itmax = 3,), (itmax = 4,), (itmax = 7,), (spd = true,), (snd = true,), (flip = true,),
               (sp = true,), (τ = 12.0, ν = -0.7), (τ = 0.0, ν = 0.0))     # sp and τ = ν = 0: what tricg! cannot take
      native(2) do; trimr!(ws, A_gpu, b, c; kw...); end
      generic(trimr!, ws2, A_gpu, b, c; kw...)
      @test ws.stats.niter == ws2.stats.niter
      @test ws.stats.status == ws2.stats.status
      @test (ws.stats.solved, ws.stats.inconsistent) == (ws2.stats.solved, ws2.stats.inconsistent)
      @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
      @test Vector(ws.y) ≈ Vector(ws2.y) rtol = 1e-6
    end
    @test_throws Exception trimr!(ws, A_gpu, b, c; spd = true, flip = true)
    @test_throws Exception trimr!(ws, A_gpu, b, c; sp = true, snd = true)
  end

  @testset "warm start, callback, verbose, M and N" begin
    ws = TrimrWorkspace(n, n, S, S)
    x0 = HIPVector(collect(range(-0.5, 0.5; length = n)))
    y0 = HIPVector(collect(range(0.25, -0.25; length = n)))
    native(2) do; trimr!(ws, A_gpu, b, c, x0, y0; τ = 12.0, ν = -0.7); end
    @test ws.stats.solved && block_residual(A_cpu, b_cpu, c_cpu, Vector(ws.x), Vector(ws.y), 12.0, -0.7) ≤ 1e-6
    seen = Int[]
    native(1) do
      trimr!(ws, A_gpu, b, c; history = true, callback = w -> (push!(seen, length(w.stats.residuals)); length(seen) == 3))
    end
    @test seen == [2, 3, 4]
    @test ws.stats.status == "user-requested exit"
    io = IOBuffer()                                                  # no file descriptor: the generic method prints
    g0 = KrylovHIP.GENERIC_SOLVES[]
    trimr!(ws, A_gpu, b, c; verbose = 1, iostream = io)
    @test KrylovHIP.GENERIC_SOLVES[] == g0 + 1
    @test occursin("TriMR: system of $(2n) equations in $(2n) variables", String(take!(io)))
  end

  @testset "rectangular and breakdown systems of the reference" begin
    for transpose in (false, true)
      Ar, br, cr, _, _ = small_sqd(transpose)
      mr, nr = size(Ar)
      ws = TrimrWorkspace(mr, nr, S, S)
      native(0) do; trimr!(ws, HIPCsr(sparse(Ar)), HIPVector(br), HIPVector(cr)); end      # m ≠ n: the primitive sequence
      @test length(ws.x) == mr && length(ws.y) == nr
      @test block_residual(Ar, br, cr, Vector(ws.x), Vector(ws.y), 1.0, -1.0) ≤ 1e-6
      Ab, bb, cb = ssy_mo_breakdown(transpose)
      Ab = Matrix{Float64}(Ab)
      ws = TrimrWorkspace(size(Ab, 1), size(Ab, 2), S, S)
      native(0) do; trimr!(ws, HIPCsr(sparse(Ab)), HIPVector(bb), HIPVector(cb)); end
      @test block_residual(Ab, bb, cb, Vector(ws.x), Vector(ws.y), 1.0, -1.0) ≤ 1e-6
      native(0) do; trimr!(ws, HIPCsr(sparse(Ab)), HIPVector(bb), HIPVector(cb); τ = 1.0, ν = 1.0); end
      @test ws.stats.inconsistent && ws.stats.status == "inconsistent linear system"
    end
    for sys in (ssy_mo_breakdown2, ssy_mo_breakdown3)
      Ab, bb, cb = sys(Float64)
      Ab = Matrix{Float64}(Ab)
      ws = TrimrWorkspace(3, 3, S, S)
      native(2) do; trimr!(ws, HIPCsr(sparse(Ab)), HIPVector(Vector{Float64}(bb)), HIPVector(Vector{Float64}(cb))); end
      @test block_residual(Ab, bb, cb, Vector(ws.x), Vector(ws.y), 1.0, -1.0) ≤ 1e-6
    end
  end
end
