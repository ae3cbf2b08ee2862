# bilq.jl -- bilq! through the specialised method (the library's device-resident loop on A and A') against the generic method of
# Krylov.jl on the same device types.  Stand-alone beside runtests.jl:
#
#   julia --project=julia/KrylovHIP julia/KrylovHIP/test/bilq.jl       (needs an MI355X and krylov.jl_amd/libkrylov_hip.so)
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

@testset "bilq! -- KrylovHIP" begin
  A_cpu, b_cpu = kron_unsymmetric(8)
  A_cpu = sparse(A_cpu)
  n = size(A_cpu, 1)
  A_gpu = HIPCsr(A_cpu)
  b = HIPVector(b_cpu)
  S = HIPVector

  @testset "bilq(A_gpu, b_gpu): the first solver call of docs/src/gpu.md" begin
    x, stats = native(2) do; bilq(A_gpu, b); end                     # forwards callback = workspace -> false
    @test stats.solved
    @test norm(b_cpu - A_cpu * Vector(x)) ≤ 1e-6 * norm(b_cpu)
    @test A_gpu' === A_gpu'                                          # A' is built once and kept on the matrix
  end

  @testset "native against generic" begin
    ws = BilqWorkspace(n, n, S); ws2 = BilqWorkspace(n, n, S)
    native(2) do; bilq!(ws, A_gpu, b; history = true); end
    generic(bilq!, ws2, A_gpu, b; history = true)
    @test ws.stats.niter == ws2.stats.niter
    @test ws.stats.status == ws2.stats.status
    @test length(ws.stats.residuals) == ws.stats.niter + 1
    @test ws.stats.residuals ≈ ws2.stats.residuals rtol = 1e-6
    @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    @test Krylov.solution(ws) === ws.x
    for kw in ((transfer_to_bicg = false,), (c = HIPVector(-b_cpu),), (itmax = 7,))
      native(2) do; bilq!(ws, A_gpu, b; kw...); end
      generic(bilq!, ws2, A_gpu, b; kw...)
      @test ws.stats.niter == ws2.stats.niter
      @test ws.stats.status == ws2.stats.status
    end
  end

  @testset "warm start, Jacobi, callback, verbose" begin
    ws = BilqWorkspace(n, n, S)
    x0 = HIPVector(collect(range(-0.5, 0.5; length = n)))
    native(2) do; bilq!(ws, A_gpu, b, x0); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    native(1) do; bilq!(ws, A_gpu, b; M = KrylovHIP.jacobi(A_gpu)); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    native(1) do; bilq!(ws, A_gpu, b; N = KrylovHIP.jacobi(A_gpu)); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    seen = Int[]
    native(1) do; bilq!(ws, A_gpu, b; history = true, callback = w -> (push!(seen, length(w.stats.residuals)); length(seen) == 3)); end
    @test seen == [2, 3, 4]
    @test ws.stats.status == "user-requested exit"
    io = IOBuffer()                                                  # no file descriptor: the generic method prints
    g0 = KrylovHIP.GENERIC_SOLVES[]
    bilq!(ws, A_gpu, b; verbose = 1, iostream = io)
    @test KrylovHIP.GENERIC_SOLVES[] == g0 + 1
    @test occursin("BILQ: system of size $n", String(take!(io)))
  end

  @testset "the reference's breakdowns" begin
    A2, b2, c2 = unsymmetric_breakdown()
    ws = BilqWorkspace(2, 2, S)
    native(2) do; bilq!(ws, HIPCsr(sparse(A2)), HIPVector(b2); c = HIPVector(c2)); end
    @test ws.stats.niter == 2 && ws.stats.solved
    @test Vector(ws.x) ≈ [0.0, 1.0] atol = 1e-12
    A3, b3, c3 = bc_breakdown()
    bilq!(ws, HIPCsr(sparse(A3)), HIPVector(b3); c = HIPVector(c3))
    @test ws.stats.niter == 0 && !ws.stats.solved
    @test ws.stats.status == "Breakdown bᴴc = 0"
  end
end
