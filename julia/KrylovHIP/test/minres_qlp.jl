# minres_qlp.jl -- minres_qlp! through the specialised method (the library's device-resident loop) against the generic method of
# Krylov.jl on the same device types.  Included from runtests.jl, and stand-alone beside it:
#
#   julia --project=julia/KrylovHIP julia/KrylovHIP/test/minres_qlp.jl     (needs an MI355X and krylov.jl_amd/libkrylov_hip.so)
using Test, LinearAlgebra, SparseArrays
using Krylov, KrylovHIP
import KrylovHIP: HIPVector, HIPCsr, CTX, Ctx

@isdefined(symmetric_inconsistent) || include(joinpath(pkgdir(Krylov), "test", "test_utils.jl"))   # symmetric_indefinite, square_inconsistent, ...
@isdefined(get_div_grad) || include(joinpath(pkgdir(Krylov), "test", "get_div_grad.jl"))

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
generic_minres_qlp(ws, A, b; kw...) = invoke(minres_qlp!, Tuple{typeof(ws),Any,AbstractVector{Float64}}, ws, A, b; kw...)

@testset "minres_qlp! -- KrylovHIP" begin
  A_cpu = get_div_grad(8, 8, 8)
  n = size(A_cpu, 1)
  b_cpu = ones(n)
  A_gpu = HIPCsr(A_cpu)
  b = HIPVector(b_cpu)
  S = HIPVector

  @testset "minres_qlp(A_gpu, b_gpu)" begin
    x, stats = native(2) do; minres_qlp(A_gpu, b); end               # forwards callback = workspace -> false
    @test stats.solved && !stats.inconsistent
    @test norm(b_cpu - A_cpu * Vector(x)) / norm(b_cpu) ≤ 1e-6 * norm(A_cpu) * norm(Vector(x))
  end

  @testset "native against generic" begin
    ws = MinresQlpWorkspace(n, n, S); ws2 = MinresQlpWorkspace(n, n, S)
    native(2) do; minres_qlp!(ws, A_gpu, b; history = true); end
    generic_minres_qlp(ws2, A_gpu, b; history = true)
    @test ws.stats.niter == ws2.stats.niter
    @test ws.stats.status == ws2.stats.status
    @test length(ws.stats.residuals) == length(ws.stats.Acond) == ws.stats.niter + 1
    @test length(ws.stats.Aresiduals) == ws.stats.niter
    @test ws.stats.residuals ≈ ws2.stats.residuals rtol = 1e-6
    @test ws.stats.Aresiduals ≈ ws2.stats.Aresiduals rtol = 1e-6
    @test ws.stats.Acond ≈ ws2.stats.Acond rtol = 1e-6
    @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    @test Krylov.solution(ws) === ws.x
    for kw in ((itmax = 1,), (itmax = 2,), (itmax = 3,), (λ = -0.5,), (atol = 0.0, rtol = 1e-10), (Artol = 1e-3,))
      native(2) do; minres_qlp!(ws, A_gpu, b; kw...); end
      generic_minres_qlp(ws2, A_gpu, b; kw...)
      @test ws.stats.niter == ws2.stats.niter
      @test ws.stats.status == ws2.stats.status
      @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    end
  end

  @testset "singular and inconsistent: the minimum-length solution" begin
    λ = -(6 - 6cos(π / 9))                                           # the smallest eigenvalue of get_div_grad(8, 8, 8), negated
    bs_cpu = sin.(1 .+ 0.37 .* (0:n-1))
    u = sin.(π .* (1:8) ./ 9); u = kron(u, u, u)
    x, stats = native(2) do; minres_qlp(A_gpu, HIPVector(bs_cpu); λ = λ); end
    @test stats.inconsistent && !stats.solved
    @test stats.status == "found approximate minimum least-squares solution"
    r = bs_cpu - A_cpu * Vector(x) - λ * Vector(x)
    @test norm(A_cpu * r + λ * r) ≤ 1e-6 * norm(A_cpu * bs_cpu + λ * bs_cpu)
    @test abs(dot(Vector(x), u)) ≤ 1e-12 * norm(Vector(x)) * norm(u)
    A1, b1 = square_inconsistent()
    x, stats = native(2) do; minres_qlp(HIPCsr(sparse(A1)), HIPVector(b1)); end
    @test stats.inconsistent
    A2, b2 = symmetric_inconsistent()
    x, stats = native(2) do; minres_qlp(HIPCsr(sparse(A2)), HIPVector(b2)); end
    r = b2 - A2 * Vector(x)
    @test stats.inconsistent && norm(A2 * r) / norm(A2 * b2) ≤ 1e-6
  end

  @testset "warm start, Jacobi, callback, verbose, linesearch" begin
    ws = MinresQlpWorkspace(n, n, S)
    x0 = HIPVector(collect(range(-0.5, 0.5; length = n)))
    native(2) do; minres_qlp!(ws, A_gpu, b, x0; atol = 0.0, rtol = 1e-10); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    native(1) do; minres_qlp!(ws, A_gpu, b; M = KrylovHIP.jacobi(A_gpu), atol = 0.0, rtol = 1e-10); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    seen = Int[]
    native(1) do; minres_qlp!(ws, A_gpu, b; history = true, callback = w -> (push!(seen, length(w.stats.residuals)); length(seen) == 2)); end
    @test seen == [2, 3]
    @test ws.stats.status == "user-requested exit"
    io = IOBuffer()                                                  # no file descriptor: the generic method prints
    g0 = KrylovHIP.GENERIC_SOLVES[]
    minres_qlp!(ws, A_gpu, b; verbose = 1, iostream = io)
    @test KrylovHIP.GENERIC_SOLVES[] == g0 + 1
    @test occursin("MINRES-QLP: system of size $n", String(take!(io)))
    A1, b1 = symmetric_indefinite()                                  # linesearch is the generic method's
    ws1 = MinresQlpWorkspace(10, 10, S)
    minres_qlp!(ws1, HIPCsr(sparse(A1)), HIPVector(b1); linesearch = true)
    @test KrylovHIP.GENERIC_SOLVES[] == g0 + 2 && ws1.stats.status == "nonpositive curvature"
  end

  @testset "indefinite with a shift, zero right-hand side" begin
    A1, b1 = symmetric_indefinite()
    x, stats = native(2) do; minres_qlp(HIPCsr(sparse(A1)), HIPVector(b1); λ = 2.0); end
    @test stats.solved && norm(b1 - (A1 + 2.0I) * Vector(x)) / norm(b1) ≤ 1e-6 * norm(A1) * norm(Vector(x))
    ws = MinresQlpWorkspace(10, 10, S)
    minres_qlp!(ws, HIPCsr(sparse(A1)), HIPVector(zeros(10)); history = true)
    @test ws.stats.status == "x is a zero-residual solution" && norm(Vector(ws.x)) == 0
    @test ws.stats.residuals == [0.0] && ws.stats.Acond == [0.0] && isempty(ws.stats.Aresiduals)
  end
end
