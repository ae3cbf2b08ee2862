# qmr.jl -- qmr! through the specialised method (the library's device-resident loop on A and A') against the generic method of
# Krylov.jl on the same device types.  Stand-alone beside runtests.jl:
#
#   julia --project=julia/KrylovHIP julia/KrylovHIP/test/qmr.jl        (needs an MI355X and krylov.jl_amd/libkrylov_hip.so)
using Test, LinearAlgebra, SparseArrays
using Krylov, KrylovHIP
import KrylovHIP: HIPVector, HIPCsr, CTX, Ctx

include(joinpath(pkgdir(Krylov), "test", "test_utils.jl"))          # kron_unsymmetric, unsymmetric_breakdown, bc_breakdown

CTX[] = Ctx(0)

generic(f!, ws, A, b; kw...) = invoke(f!, Tuple{typeof(ws),Any,AbstractVector{Float64}}, ws, A, b; kw...)
function native(body, path::Integer)
  n0 = KrylovHIP.NATIVE_SOLVES[]; g0 = KrylovHIP.GENERIC_SOLVES[]
  out = body()
  @test KrylovHIP.NATIVE_SOLVES[] == n0 + 1
  @test KrylovHIP.GENERIC_SOLVES[] == g0
  @test KrylovHIP.LAST_PATH[] == path
  out
end

@testset "qmr! -- KrylovHIP" begin
  A_cpu, b_cpu = kron_unsymmetric(8)
  A_cpu = sparse(A_cpu)
  n = size(A_cpu, 1)
  A_gpu = HIPCsr(A_cpu)
  b = HIPVector(b_cpu)
  S = HIPVector

  @testset "qmr(A_gpu, b_gpu)" begin
    x, stats = native(2) do; qmr(A_gpu, b); end                      # forwards callback = workspace -> false
    @test stats.solved
    @test norm(b_cpu - A_cpu * Vector(x)) ≤ 1e-6 * norm(b_cpu)
    @test A_gpu' === A_gpu'                                          # A' is built once and kept on the matrix
  end

  @testset "native against generic" begin
    ws = QmrWorkspace(n, n, S); ws2 = QmrWorkspace(n, n, S)
    native(2) do; qmr!(ws, A_gpu, b; history = true); end
    generic(qmr!, ws2, A_gpu, b; history = true)
    @test ws.stats.niter == ws2.stats.niter
    @test ws.stats.status == ws2.stats.status
    @test length(ws.stats.residuals) == ws.stats.niter + 1
    @test ws.stats.residuals ≈ ws2.stats.residuals rtol = 1e-6
    @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    @test Krylov.solution(ws) === ws.x
    for kw in ((c = HIPVector(-b_cpu),), (itmax = 1,), (itmax = 2,), (itmax = 7,))
      native(2) do; qmr!(ws, A_gpu, b; kw...); end
      generic(qmr!, ws2, A_gpu, b; kw...)
      @test ws.stats.niter == ws2.stats.niter
      @test ws.stats.status == ws2.stats.status
      @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    end
  end

  @testset "warm start, Jacobi, callback, verbose" begin
    ws = QmrWorkspace(n, n, S)
    x0 = HIPVector(collect(range(-0.5, 0.5; length = n)))
    native(2) do; qmr!(ws, A_gpu, b, x0); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    native(1) do; qmr!(ws, A_gpu, b; M = KrylovHIP.jacobi(A_gpu)); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    native(1) do; qmr!(ws, A_gpu, b; N = KrylovHIP.jacobi(A_gpu)); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    seen = Int[]
    native(1) do; qmr!(ws, A_gpu, b; history = true, callback = w -> (push!(seen, length(w.stats.residuals)); length(seen) == 3)); end
    @test seen == [2, 3, 4]
    @test ws.stats.status == "user-requested exit"
    io = IOBuffer()                                                  # no file descriptor: the generic method prints
    g0 = KrylovHIP.GENERIC_SOLVES[]
    qmr!(ws, A_gpu, b; verbose = 1, iostream = io)
    @test KrylovHIP.GENERIC_SOLVES[] == g0 + 1
    @test occursin("QMR: system of size $n", String(take!(io)))
  end

  @testset "the reference's breakdowns" begin
    A2, b2, c2 = unsymmetric_breakdown()
    ws = QmrWorkspace(2, 2, S)
    native(2) do; qmr!(ws, HIPCsr(sparse(A2)), HIPVector(b2); c = HIPVector(c2), history = true); end
    @test ws.stats.niter == 2 && ws.stats.solved
    @test Vector(ws.x) ≈ [0.0, 1.0] atol = 1e-12
    @test ws.stats.residuals ≈ [1.0, √2, 0.0] atol = 1e-12
    A3, b3, c3 = bc_breakdown()
    qmr!(ws, HIPCsr(sparse(A3)), HIPVector(b3); c = HIPVector(c3))
    @test ws.stats.niter == 0 && !ws.stats.solved
    @test ws.stats.status == "Breakdown bᴴc = 0"
  end
end
