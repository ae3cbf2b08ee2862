# symmlq.jl -- symmlq! through the specialised method (the library's device-resident loop) against the generic method of Krylov.jl on
# the same device types.  Included from runtests.jl, and stand-alone beside it:
#
#   julia --project=julia/KrylovHIP julia/KrylovHIP/test/symmlq.jl     (needs an MI355X and krylov.jl_amd/libkrylov_hip.so)
using Test, LinearAlgebra, SparseArrays
using Krylov, KrylovHIP
import KrylovHIP: HIPVector, HIPCsr, CTX, Ctx

@isdefined(symmetric_breakdown) || include(joinpath(pkgdir(Krylov), "test", "test_utils.jl"))   # symmetric_indefinite, symmetric_breakdown
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
generic_symmlq(ws, A, b; kw...) = invoke(symmlq!, Tuple{typeof(ws),Any,AbstractVector{Float64}}, ws, A, b; kw...)
same_missing(a, b) = ismissing.(a) == ismissing.(b)

@testset "symmlq! -- KrylovHIP" begin
  A_cpu = get_div_grad(8, 8, 8)
  n = size(A_cpu, 1)
  b_cpu = ones(n)
  A_gpu = HIPCsr(A_cpu)
  b = HIPVector(b_cpu)
  S = HIPVector

  @testset "symmlq(A_gpu, b_gpu)" begin
    x, stats = native(2) do; symmlq(A_gpu, b); end                   # forwards callback = workspace -> false
    @test stats.solved
    @test norm(b_cpu - A_cpu * Vector(x)) / norm(b_cpu) ≤ 1e-6 * norm(A_cpu) * norm(Vector(x))
  end

  @testset "native against generic" begin
    ws = SymmlqWorkspace(n, n, S); ws2 = SymmlqWorkspace(n, n, S)
    native(2) do; symmlq!(ws, A_gpu, b; history = true); end
    generic_symmlq(ws2, A_gpu, b; history = true)
    @test ws.stats.niter == ws2.stats.niter
    @test ws.stats.status == ws2.stats.status
    @test length(ws.stats.residuals) == length(ws.stats.residualscg) == ws.stats.niter + 1
    @test ws.stats.residuals ≈ ws2.stats.residuals rtol = 1e-6
    @test same_missing(ws.stats.residualscg, ws2.stats.residualscg)
    @test collect(skipmissing(ws.stats.residualscg)) ≈ collect(skipmissing(ws2.stats.residualscg)) rtol = 1e-6
    @test isempty(ws.stats.errors) && isempty(ws.stats.errorscg)
    @test ws.stats.Anorm ≈ ws2.stats.Anorm && ws.stats.Acond ≈ ws2.stats.Acond
    @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    @test Krylov.solution(ws) === ws.x
    for kw in ((transfer_to_cg = false,), (itmax = 1,), (itmax = 3,), (λ = -0.5,), (atol = 0.0, rtol = 1e-10))
      native(2) do; symmlq!(ws, A_gpu, b; kw...); end
      generic_symmlq(ws2, A_gpu, b; kw...)
      @test ws.stats.niter == ws2.stats.niter
      @test ws.stats.status == ws2.stats.status
      @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    end
  end

  @testset "error estimates" begin                                   # test/test_symmlq.jl:46-62; λest ≠ 0 runs the host-driven loop
    λest = (1 - 1e-10) * eigmin(Matrix(A_cpu))
    x_exact = Matrix(A_cpu) \ b_cpu
    for window in (1, 5)
      x, stats = native(1) do; symmlq(A_gpu, b; λest = λest, window = window, transfer_to_cg = false, history = true); end
      @test norm(x_exact - Vector(x)) ≤ stats.errors[end]
      @test length(stats.errors) == length(stats.errorscg) == stats.niter + 1
      @test !any(ismissing, stats.errorscg)
    end
  end

  @testset "warm start, Jacobi, callback, verbose" begin
    ws = SymmlqWorkspace(n, n, S)
    x0 = HIPVector(collect(range(-0.5, 0.5; length = n)))
    native(2) do; symmlq!(ws, A_gpu, b, x0; atol = 0.0, rtol = 1e-10); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    native(1) do; symmlq!(ws, A_gpu, b; M = KrylovHIP.jacobi(A_gpu), atol = 0.0, rtol = 1e-10); end
    @test ws.stats.solved && norm(b_cpu - A_cpu * Vector(ws.x)) ≤ 1e-6 * norm(b_cpu)
    seen = Int[]
    native(1) do; symmlq!(ws, A_gpu, b; history = true, callback = w -> (push!(seen, length(w.stats.residuals)); length(seen) == 2)); end
    @test seen == [2, 3]
    @test ws.stats.status == "user-requested exit"
    io = IOBuffer()                                                  # no file descriptor: the generic method prints
    g0 = KrylovHIP.GENERIC_SOLVES[]
    symmlq!(ws, A_gpu, b; verbose = 1, iostream = io)
    @test KrylovHIP.GENERIC_SOLVES[] == g0 + 1
    @test occursin("SYMMLQ: system of size $n", String(take!(io)))
  end

  @testset "indefinite, breakdown, zero right-hand side" begin
    A1, b1 = symmetric_indefinite()
    x, stats = native(2) do; symmlq(HIPCsr(sparse(A1)), HIPVector(b1)); end
    @test stats.solved && norm(b1 - A1 * Vector(x)) / norm(b1) ≤ 1e-6 * norm(A1) * norm(Vector(x))
    A2, b2 = symmetric_breakdown()
    ws = SymmlqWorkspace(2, 2, S)
    native(2) do; symmlq!(ws, HIPCsr(sparse(A2)), HIPVector(b2); history = true); end
    @test ws.stats.solved && Vector(ws.x) == [0.0, 1.0]
    @test ws.stats.status == "solution xᶜ good enough given atol and rtol"
    @test ismissing(ws.stats.residualscg[1]) && !ismissing(ws.stats.residualscg[2])
    symmlq!(ws, HIPCsr(sparse(A2)), HIPVector(zeros(2)))
    @test ws.stats.status == "x is a zero-residual solution" && norm(Vector(ws.x)) == 0
    @test isnan(ws.stats.Anorm) && isnan(ws.stats.Acond)
  end
end
